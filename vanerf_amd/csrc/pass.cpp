// pass.cpp -- vanerf_render_pass: one whole pass of the hot path as a single C entry point (reference
// VANeRF.batch_render_pifu_nerf, src/model.py:1102-1360).  Host-side sequencing only: it enqueues the library's own entry points
// on the caller's stream, in the order vanerf_amd/renderer.py:render_pass does, with every temporary carved out of one
// caller-provided scratch block -- no allocation, no host synchronisation, nothing kept between calls.
#include "common.h"

#include <cstdlib>

using namespace vanerf;

namespace {

constexpr int64_t ALIGN = 256;
constexpr int64_t PARTITION_MIN_SAMPLES = 1 << 18; // as renderer.PARTITION_MIN_SAMPLES: below it the three partition kernels cost more than they save

struct Carver {
    char* base;
    int64_t off = 0;
    explicit Carver(void* b) : base(static_cast<char*>(b)) {}
    template <class T> T* take(int64_t n)
    {
        T* p = base ? reinterpret_cast<T*>(base + off) : nullptr;
        off += ((n * (int64_t)sizeof(T) + ALIGN - 1) / ALIGN) * ALIGN;
        return p;
    }
};

// The temporaries of a pass.  Laid out by the same code for the size query (base == NULL) and for the run.
struct Layout {
    float *rays_d, *cam_pos, *near, *far, *pts, *q_sdf_c, *rgba_c, *contrib, *z_new, *q_sdf_f, *rgba_f, *z_fine, *color_f3, *s1;
    float *raw_c, *rgba_cf;      // noisy reuse: the coarse points' raw outputs, and their eval_func with the fine batch's draws
    uint8_t *valid_c, *valid_f;
    uint8_t *q_vis;
    int32_t *knn, *order, *src, *tile_order;
    int64_t tile_order_slots;
    unsigned long long* queue_words; // work-queue heads of the pass's four big launches (mesh query and per-sample networks, coarse and fine)
    void* order_scratch;
    int64_t order_scratch_bytes, total;
};

// reuse: 0 the fine march evaluates all Sc + Sf samples; 1 it evaluates the Sf new ones and the composite gathers the coarse evaluations;
// 2 the same under per-sample noise: raw network outputs once per point, eval_func once per set of draws (vanerf_eval_func)
Layout carve(void* base, int R, int Sc, int Sf, int fine, int reuse, int n_views)
{
    Carver c(base);
    Layout L{};
    const int64_t nc = (int64_t)R * Sc, nf = fine ? (int64_t)R * (reuse ? Sf : Sc + Sf) : 0, nmax = nc > nf ? nc : nf;
    L.queue_words = c.take<unsigned long long>(4);
    L.rays_d = c.take<float>(3LL * R);
    L.cam_pos = c.take<float>(4LL * n_views); // [n_views][4]
    L.near = c.take<float>(R);
    L.far = c.take<float>(R);
    L.pts = c.take<float>(3 * nmax);
    L.q_vis = c.take<uint8_t>(nmax);
    L.knn = c.take<int32_t>(nmax);
    L.order = c.take<int32_t>(nmax);
    L.order_scratch_bytes = vanerf_query_order_scratch(nmax);
    L.order_scratch = c.take<uint8_t>(L.order_scratch_bytes);
    // The mesh query's item order (vanerf_mesh_tile_order) pads every 8 x 8 pixel tile to 64 rays, and L.order is still needed behind it.  The
    // size query does not know the grid's sides: a quarter on top holds any grid with both sides >= 64 or multiples of 8; a launch whose
    // table would not fit (small, ragged grids) keeps the index grouping.
    L.tile_order_slots = (5 * nmax + 3) / 4;
    L.tile_order = c.take<int32_t>(L.tile_order_slots);
    L.q_sdf_c = c.take<float>(nc);
    L.rgba_c = c.take<float>(5 * nc);
    L.contrib = c.take<float>(nc);
    if (fine) {
        L.z_new = c.take<float>((int64_t)R * Sf);
        L.src = c.take<int32_t>((int64_t)R * (Sc + Sf));
        L.z_fine = c.take<float>((int64_t)R * (Sc + Sf));
        L.q_sdf_f = c.take<float>(nf);
        L.rgba_f = c.take<float>(5 * nf);
        if (reuse == 2) {
            L.raw_c = c.take<float>(5 * nc);
            L.rgba_cf = c.take<float>(5 * nc);
            L.valid_c = c.take<uint8_t>(nc);
            L.valid_f = c.take<uint8_t>(nf);
        }
    }
    L.color_f3 = c.take<float>(3LL * R); // stand-ins for optional outputs the caller did not ask for
    L.s1 = c.take<float>(4LL * R);
    L.total = c.off;
    return L;
}

constexpr int MESH_TILE_ORDER_MAX_S = 128; // vanerf_mesh_tile_order sorts a tile in LDS: it refuses more samples per ray
constexpr int MESH_TILE_ORDER_DEFAULT = 3;

// VANERF_MESH_TILE_ORDER (read at every pass, for tests and A/B runs): which mesh launches group their tiles' samples by depth.  0: none (the
// index grouping), 1: the coarse launch, 2: the fine launch, 3: both; unset or anything else: the default.  The results do not depend on it.
int mesh_tile_order_mode()
{
    const char* e = std::getenv("VANERF_MESH_TILE_ORDER");
    return (e && e[0] >= '0' && e[0] <= '3' && !e[1]) ? e[0] - '0' : MESH_TILE_ORDER_DEFAULT;
}

void ok(int rc, const char* what)
{
    if (rc != VANERF_OK) {
        const std::string inner = vanerf_last_error();
        throw Error(rc, std::string("vanerf_render_pass: ") + what + ": " + inner);
    }
}

// Everything of a pass behind its ray setup: the marches, the composites and the importance merge over the R rays whose directions, origins,
// clip range and coarse depths (o.z) are in place.  Nothing here knows about cameras except the per-view ray origin.
void run_marches(const VanerfWeights* w, const VanerfFrame* frame, const VanerfMeshAccel* accel, const float* verts, int nv, const int32_t* faces, int nf,
                 const VanerfPassDesc& d, int reuse, const float* vertex_products, const Layout& L, const VanerfPassOut& o, void* stream)
{
    const int R = d.n_views * d.nx * d.ny, Sc = d.Sc, Sf = d.Sf;
    const int rays_per_view = d.cams ? d.nx * d.ny : 0; // 0: one origin L.cam_pos[3] for every ray; else ray r starts at L.cam_pos[r / rays_per_view][4]
    // ray-grid hint of the mesh query (0, 0 with a pixel list: none); the views of a pass stack their rows: (nx, n_views * ny)
    const int grid_nx = d.pixels_xy ? 0 : d.nx, grid_ny = d.pixels_xy ? 0 : d.n_views * d.ny;
    // one march: points, mesh query (+ 1-NN), validity partition, per-sample networks
    int marches = 0; // every launch with a work queue gets a word of its own from the scratch block (nothing is shared between launches in flight)
    const int tile_order_mode = mesh_tile_order_mode();
    auto march = [&](const float* z, int S, const float* noise, float* q_sdf, float* rgba, uint8_t* valid_raw = nullptr) { // valid_raw: raw outputs + flags
        const bool fine_launch = marches > 0;
        unsigned long long* const qw = L.queue_words + 2 * marches++;
        const int64_t n = (int64_t)R * S;
        ok(vanerf_sample_points(L.rays_d, L.cam_pos, z, R, rays_per_view, S, L.pts, stream), "sample points");
        // the tile's samples in depth order (z: the depths L.pts were just made from); a table that does not fit: no order, same results
        const int32_t* tile_order = nullptr;
        const int64_t slots = (int64_t)((grid_nx + 7) / 8) * ((grid_ny + 7) / 8) * 64 * S;
        if (grid_nx && S <= MESH_TILE_ORDER_MAX_S && slots <= L.tile_order_slots && (tile_order_mode & (fine_launch ? 2 : 1))) {
            ok(vanerf_mesh_tile_order(z, grid_nx, grid_ny, S, L.tile_order, stream), "mesh tile order");
            tile_order = L.tile_order;
        }
        ok(vanerf_mesh_query_accel_ordered(accel, verts, nv, faces, nf, frame->vert_vis, L.pts, n, q_sdf, L.q_vis, nullptr, L.knn, grid_nx, grid_ny,
                                           grid_nx ? S : 0, qw, tile_order, stream), "mesh query");
        const int32_t* order = nullptr;
        if (n >= PARTITION_MIN_SAMPLES) {
            ok(vanerf_query_order(frame, L.pts, n, L.order, L.order_scratch, L.order_scratch_bytes, stream), "validity partition");
            order = L.order;
        }
        ok(vanerf_query_samples(w, frame, L.pts, q_sdf, L.q_vis, L.knn, noise, order, valid_raw ? 1 : 0, n, rgba, valid_raw, qw + 1, vertex_products, stream),
           "per-sample networks");
    };
    if (reuse == 2) { // the networks once per point; eval_func with the coarse draws here, with the fine batch's draws below
        march(o.z, Sc, nullptr, L.q_sdf_c, L.raw_c, L.valid_c);
        ok(vanerf_eval_func(L.raw_c, L.valid_c, nullptr, nullptr, nullptr, d.noise_c, Sc, 0, R, frame->invalid_sdf, L.rgba_c, nullptr, stream), "eval_func (coarse)");
    } else {
        march(o.z, Sc, d.noise_c, L.q_sdf_c, L.rgba_c);
    }
    ok(vanerf_composite_handle(w, L.rgba_c, o.z, L.q_sdf_c, Sc, nullptr, nullptr, 0, nullptr, R, o.color, o.depth, o.alpha, L.s1, L.contrib, stream), "composite");
    if (!d.fine) return;
    float* z_fine = o.z_fine ? o.z_fine : L.z_fine;
    float* cf = o.color_fine ? o.color_fine : L.color_f3;
    float* df = o.depth_fine ? o.depth_fine : L.s1 + R;
    float* af = o.alpha_fine ? o.alpha_fine : L.s1 + 2LL * R;
    float* sf = o.sdf ? o.sdf : L.s1 + 3LL * R;
    ok(vanerf_importance_merge(L.contrib, o.z, d.u, d.u ? nullptr : d.t_lin_f, R, Sc, Sf, L.z_new, z_fine, L.src, nullptr, stream), "importance sampling");
    if (reuse == 2) {
        march(L.z_new, Sf, nullptr, L.q_sdf_f, L.rgba_f, L.valid_f);
        // noise_f holds one draw per position of the merged order (the reference draws them for the re-evaluated fine batch, src/model.py:1155-1156)
        ok(vanerf_eval_func(L.raw_c, L.valid_c, L.rgba_f, L.valid_f, L.src, d.noise_f, Sc, Sf, R, frame->invalid_sdf, L.rgba_cf, L.rgba_f, stream), "eval_func (fine)");
        ok(vanerf_composite_handle(w, L.rgba_cf, z_fine, L.q_sdf_c, Sc, L.rgba_f, L.q_sdf_f, Sf, L.src, R, cf, df, af, sf, nullptr, stream), "fine composite");
    } else if (reuse) {
        march(L.z_new, Sf, nullptr, L.q_sdf_f, L.rgba_f);
        ok(vanerf_composite_handle(w, L.rgba_c, z_fine, L.q_sdf_c, Sc, L.rgba_f, L.q_sdf_f, Sf, L.src, R, cf, df, af, sf, nullptr, stream), "fine composite");
    } else {
        march(z_fine, Sc + Sf, d.noise_f, L.q_sdf_f, L.rgba_f);
        ok(vanerf_composite_handle(w, L.rgba_f, z_fine, L.q_sdf_f, Sc + Sf, nullptr, nullptr, 0, nullptr, R, cf, df, af, sf, nullptr, stream), "fine composite");
    }
}

// samples per ray of the largest march of a pass (held against VIEWS_MAX_ITEMS)
int s_max(int Sc, int Sf, bool fine, bool reuse) { return !fine ? Sc : reuse ? (Sc > Sf ? Sc : Sf) : Sc + Sf; }

} // namespace

extern "C" int64_t vanerf_render_pass_scratch(int n_views, int rays_per_view, int Sc, int Sf, int fine, int reuse_coarse)
{
    if (n_views <= 0 || rays_per_view <= 0 || Sc <= 0 || Sf < 0) return 0;
    if ((long long)n_views * rays_per_view * s_max(Sc, Sf, fine != 0, reuse_coarse != 0) >= VIEWS_MAX_ITEMS) return 0; // as the pass itself
    return carve(nullptr, n_views * rays_per_view, Sc, Sf, fine, reuse_coarse, n_views).total;
}

// check, carve, ray setup, marches
extern "C" int vanerf_render_pass(const VanerfWeights* w, const VanerfFrame* frame, const VanerfMeshAccel* accel, const float* verts, int nv,
                                  const int32_t* faces, int nf, const VanerfPassDesc* desc, const VanerfPassOut* out, void* scratch,
                                  int64_t scratch_bytes, const float* vertex_products, void* stream)
{
    return guarded([&] {
        if (!w || !frame || !accel || !verts || !faces || !desc || !out || !scratch) throw_error("vanerf_render_pass: null argument");
        const VanerfPassDesc& d = *desc;
        const VanerfPassOut& o = *out;
        const int V = d.n_views, Sc = d.Sc, Sf = d.Sf;
        const bool fine = d.fine != 0;
        if (V <= 0 || d.nx <= 0 || d.ny <= 0 || Sc < 2 || (fine && Sf < 1))
            throw_error("vanerf_render_pass: n_views=%d nx=%d ny=%d Sc=%d Sf=%d", V, d.nx, d.ny, Sc, Sf);
        check_camera_source("vanerf_render_pass", d);
        if (d.cams && (d.noise_c || d.noise_f)) throw_error("vanerf_render_pass: noise_c / noise_f with a camera table (cams): the table form is the evaluation form");
        if (fine && d.noise_c && !d.noise_f) throw_error("vanerf_render_pass: noise_c without noise_f");
        const int reuse = !d.reuse_coarse || !fine ? 0 : d.noise_c ? 2 : 1;
        const int S_max = s_max(Sc, Sf, fine, reuse != 0);
        if ((long long)V * d.nx * d.ny * S_max >= VIEWS_MAX_ITEMS)
            throw_error("vanerf_render_pass: %d views of %d x %d rays at %d samples do not fit a 32-bit sample index", V, d.nx, d.ny, S_max);
        if (!o.index || !o.hit || !o.z || !o.color || !o.depth || !o.alpha) throw_error("vanerf_render_pass: a coarse output pointer is null");
        if (!d.t_lin_c || (fine && !d.u && !d.t_lin_f)) throw_error("vanerf_render_pass: linspace tables missing");
        const Layout L = carve(scratch, V * d.nx * d.ny, Sc, Sf, fine, reuse, V);
        if (scratch_bytes < L.total)
            throw_error("vanerf_render_pass: scratch of %lld bytes, %lld needed (vanerf_render_pass_scratch)", (long long)scratch_bytes, (long long)L.total);
        // a1-a4: pixel grid, rays, bbox clip, coarse depths
        ok(vanerf_ray_setup(desc, o.index, L.rays_d, L.cam_pos, L.near, L.far, o.hit, o.z, stream), "ray setup");
        run_marches(w, frame, accel, verts, nv, faces, nf, d, reuse, vertex_products, L, o, stream);
    });
}
