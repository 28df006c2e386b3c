/*
 * vanerf_hip.h -- C ABI of the MI355X-native VANeRF volume-rendering hot path (libvanerf_hip.so).
 *
 * The reference (XuanHuang0/VANeRF) has no FFI of its own: its seam is Python methods on
 * `class VANeRF(torch.nn.Module)` (src/model.py:604).  Each entry point below replaces the
 * arithmetic of one of those methods (cited per function); `vanerf_amd/model.py` keeps the
 * Python signatures and calls these through ctypes.  INTEGRATION.md shows the binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every `const float*` / `float*` / `int*` below is a DEVICE pointer borrowed from the caller
 *     (contiguous, fp32 / int32 / uint8); the library allocates nothing that outlives a call
 *     except the packed-weight handle;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); no entry point
 *     synchronises the host, all work is enqueued on `stream`;
 *   - return value: 0 on success, negative on error (message via vanerf_last_error(), thread local);
 *   - B = V = 1 (one target view, one source view): the non-spconv reference path is
 *     structurally single-view (src/networks.py:86,94) and evaluates batch items in Python loops.
 *     A VanerfPassDesc with a camera table marches several TARGET views of the one source view in one pass.
 */
#ifndef VANERF_HIP_H
#define VANERF_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VANERF_ABI_VERSION 12

#define VANERF_OK 0
#define VANERF_EINVAL (-22)
#define VANERF_ENOMEM (-12)
#define VANERF_EHIP (-5)

#define VANERF_NV 1558      /* vertices: 2 x (778 + 1 seal vertex), src/networks.py:25 */
#define VANERF_NV_HAND 779
#define VANERF_NKPT 42
#define VANERF_PE_LEVELS 3  /* sp_level, configs/vanerf.json:50 */

/* Host pointers to the per-sample network weights in the reference's state_dict layout
 * (row-major [out][in], Conv1d k=1 weights with the trailing 1 dropped).  Weight-normed layers
 * (src/utils.py:674-675) are passed as (v, g): the packer folds W = g * v / ||v||_row.          */
typedef struct {
    const float* geo_at0_w1;   /* [10][196]  geo_vis_fusion.fconv_at.0.weight   (src/networks.py:47-52) */
    const float* geo_at0_w2;   /* [3][10]    geo_vis_fusion.fconv_at.2.weight */
    const float* geo_ated0_w1; /* [64][196]  geo_vis_fusion.fconv_ated.0.weight (54-58) */
    const float* geo_ated0_w2; /* [64][64]   geo_vis_fusion.fconv_ated.2.weight */
    const float* geo_at1_w1;   /* [10][28]   geo_vis_fusion.fconv_at1.0.weight  (60-65) */
    const float* geo_at1_w2;   /* [3][10] */
    const float* geo_ated1_w1; /* [8][28]    geo_vis_fusion.fconv_ated1.0.weight (67-71) */
    const float* geo_ated1_w2; /* [8][8] */
    /* mlp_geo (src/utils.py:609-649): layers1 = [358->128, 128->128, 136->120, 120->64], layers2 = [128->64, 64->64, 64->2] */
    const float* l1_v[3];      /* weight_v of layers1.{0,1,2}: [128][358], [128][128], [120][136] */
    const float* l1_g[3];      /* weight_g: [128], [128], [120] */
    const float* l1_b[3];      /* bias */
    const float* l1_w3;        /* [64][120] layers1.3 (plain) */
    const float* l1_b3;        /* [64] */
    const float* l2_v[2];      /* layers2.{0,1}: [64][128], [64][64] */
    const float* l2_g[2];
    const float* l2_b[2];
    const float* l2_w2;        /* [2][64] layers2.2 (plain) */
    const float* l2_b2;        /* [2] */
    const float* ibr_w;        /* [24][128] ibr_compress_gfeat (src/model.py:633-636) */
    const float* ibr_b;        /* [24] */
    const float* tex_at_w1;    /* [96][96]  tex_vis_fusion.fconv_at.0.weight (src/networks.py:230-235) */
    const float* tex_at_w2;    /* [6][96] */
    const float* tex_w1;       /* [96][96]  tex_vis_fusion.fconv.0.weight (224-228) */
    const float* tex_w2;       /* [40][96]  (only rows 0..2 reach the image at V = 1: src/model.py:1613,1635) */
    float sigmoid_beta;        /* VANeRF.sigmoid_beta (src/model.py:614); clamped to >= 2e-3 as in sdf_activation (880) */
} VanerfWeightTable;

/* Per-source-frame inputs of the per-sample networks (all device pointers, fp32). */
typedef struct {
    const float* geo0;      /* [h0][w0][64] feat_geo[0], channel-last          (src/model.py:826, 971) */
    const float* geo1;      /* [h1][w1][8]  feat_geo[1], channel-last */
    const float* tex;       /* [ht][wt][8]  feat_tex, channel-last             (src/model.py:919, 972) */
    const float* img;       /* [hi][wi][4]  source image rgb + pad             (src/model.py:906) */
    const float* mask;      /* [hi][wi]     src_foreground_mask                (src/model.py:800) */
    int h0, w0, h1, w1, ht, wt, hi, wi;
    const float* verts;     /* [NV][4] vert_world xyz + pad */
    const float* vfeat0;    /* [NV][64] feat_sample(feat_geo[0], vert_xy) * vert_vis   (src/networks.py:83, 29) */
    const float* vfeat1;    /* [NV][8]  feat_sample(feat_geo[1], vert_xy) * vert_vis   (src/networks.py:96) */
    const float* vfeat_tex; /* [NV][32] [img3 | tex8 | gf18 | 0 0 0] * vert_vis        (src/networks.py:270-279) */
    const float* vert_vis;  /* [NV]     {0,1}                                          (mesh_util.py:284-318) */
    const float* kpt_cam;   /* [42][4]  key points in source-camera coordinates (src/spatial.py:84) */
    float KRT[12];          /* source view K*[R|t], rows 0..2 (src/model.py:780) */
    float extrin[12];       /* source view [R|t]                (src/spatial.py:71-72) */
    float width, height, znear, zfar; /* cam_in (src/model.py:313-317) */
    float invalid_sdf;      /* 0.1 / nml_scale (src/model.py:1144) */
    float pe_scale, pe_inv_2sigma2; /* sp_args.scale, 1/(2 sigma^2) (src/spatial.py:110-113) */
} VanerfFrame;

typedef struct VanerfWeights VanerfWeights; /* opaque device-resident packed weights */

int vanerf_abi_version(void);
const char* vanerf_last_error(void);

/* Packs the weight table into MFMA fragment order on the device.  mode selects the arithmetic of the 20 dense layers that
 * vanerf_query_samples runs with these weights:
 *   0  fp32:   v_mfma_f32_32x32x2_f32 on fp32 weights and activations (summation order is the only difference to the reference)
 *   1  bf16x3: v_mfma_f32_32x32x16_bf16, fp32 accumulate, W = W_hi + W_lo and X = X_hi + X_lo (bf16 each), three products per term;
 *              outputs within 3.3e-5 of mode 0 on the 10.9 M-sample benchmark launch, about twice as fast */
int vanerf_weights_pack(const VanerfWeightTable* w, int mode, VanerfWeights** out);
int vanerf_weights_free(VanerfWeights* w);
/* Re-packs a handle IN PLACE from parameters that live on the DEVICE (the training step: the optimiser has just changed them).  `dev` is a
 * weight table of device pointers to the parameters' own storage (fp32, contiguous); sigmoid_beta_dev points at the parameter on the device
 * (NULL: dev->sigmoid_beta, a host value, is taken).  A few launches on `stream`, no copy to the host, no allocation after the first call, nothing
 * blocks; the streams are bit-identical to a fresh vanerf_weights_pack of the same values.  The caller orders the update after the launches
 * that still read the old weights (same stream, or an event).                                                                                  */
int vanerf_weights_update(VanerfWeights* w, const VanerfWeightTable* dev, const float* sigmoid_beta_dev, void* stream);
/* Diagnostics: number of 32-sample groups (since the pack) for which vanerf_query_samples took its all-invalid short path
 * (only the colour branch evaluated).  Blocking device read; for benchmarks and tests.                                        */
int vanerf_weights_short_groups(const VanerfWeights* w, uint64_t* count);
/* Host-only view of the packed fragment stream (no GPU touched): out[cap] or NULL to query the size; offsets[20]. */
int vanerf_weights_pack_host(const VanerfWeightTable* w, float* out, int64_t cap, int64_t* n_out, unsigned* offsets);
/* The streams a handle can carry: the `which` of the two calls below.  An fp32 handle carries FP32 and BACKWARD, a bf16x3 handle the others. */
enum {
    VANERF_STREAM_FP32 = 0,       /* the fp32 forward stream */
    VANERF_STREAM_BF16X3 = 1,     /* the bf16x3 forward stream (32-bit words of two bf16 each, copied raw) */
    VANERF_STREAM_BACKWARD = 2,   /* the transposed fp32 stream of the fused backward pass */
    VANERF_STREAM_HOISTED = 3,    /* the hoisted bf16x3 stream behind stream 1 (three first layers packed with their per-sample k-pairs only) */
    VANERF_STREAM_LEAN = 4,       /* the lean bf16x3 stream behind that (what vanerf_query_samples runs on when it is given vertex_products: the
                                   * hoisted stream with geo_vis_fusion.fconv_ated.2 / fconv_ated1.2 multiplied into mlp_geo.layers1's layers 0 / 2,
                                   * no bias k-pair in five layers, one k-pair less in TexVisFusion's input) */
    VANERF_STREAM_LEAN_BIAS = 5,  /* the lean stream's fp32 bias table (five layers' biases in accumulator-register order) */
    VANERF_STREAM_LEAN_FOLDED = 6 /* its two folded matrices in fp32 ([128][64], then [120][8]) */
};
/* Host-only view of any stream a handle can carry.  out[cap] or NULL: the size. */
int vanerf_weights_stream_host(const VanerfWeightTable* w, int which, float* out, int64_t cap, int64_t* n_out);
/* The streams a handle holds on the device, copied back to host memory (blocking; for tests of vanerf_weights_update): which = 0 the forward
 * stream of the handle's mode (never 1), any other a stream the handle carries.                                                               */
int vanerf_weights_download(const VanerfWeights* w, int which, float* out, int64_t cap, int64_t* n_out);

/* a1-a4  Pixel grid, ray generation, bbox clipping, coarse depths (src/model.py:1191-1238, 1496-1570), described by a VanerfPassDesc (below).
 *   Read: x0, y0, step_x, step_y, y_block, nx, ny, pixels_xy, row_blocks, width, n_views, cams or invK_T / RT / znear / zfar, bounds, Sc,
 *   t_lin_c and jitter.  The other fields are ignored.
 *   grid: x = x0 + ix*step_x, y = y0 + (iy / y_block)*step_y + (iy % y_block)*step_x for iy < ny (outer), ix < nx (inner); nx*ny rays per view
 *         (the reference's strided grid: step_x = step_y = 2^(level-1), y_block = 1, model.py:1194; a multi-GPU shard takes blocks of
 *          y_block = 8 consecutive rows, step_x = 1, step_y = 8 N, y0 = 8 rank: 8x8 pixel tiles stay whole, the load stays balanced)
 *   row_blocks: the rows as a list of blocks instead, row iy = row_blocks[iy / y_block] + (iy % y_block) * step_x (device table of ny / y_block
 *         entries; ny a whole number of blocks): the shard of a multi-GPU view whose blocks of 8 rows were dealt by cost instead of round
 *         robin (vanerf_amd/parallel.py: deal_blocks)
 *   pixels_xy: an explicit pixel list [nx*ny][2] instead of a grid (the grid fields are ignored): the training branch's clamped 64x64 window
 *         around a random mask pixel (src/model.py:1172-1189) is not a regular grid
 *   camera: cams == NULL: invK_T[9] = inverse(K[:3,:3]) transposed, row-major (host computed, as th.inverse at model.py:1208), RT[12] = target
 *         [R|t] rows 0..2, znear, zfar, by value; n_views = 1.  Else cams[n_views][24] (DEVICE, fp32) = invK_T[9], RT[12], znear, zfar, one pad
 *         per view, n_views in [1, 65535]: every view has the same grid (plain: no pixel list, no row blocks, y_block = 1) and width, and
 *         n_views * nx * ny * Sc must stay below 2^31 - 1 (the 32-bit sample index of vanerf_query_order).  Ray v * nx * ny + iy * nx + ix of
 *         the outputs is ray (ix, iy) of view v, with the bits the by-value form gives for that camera alone (one ray function behind both).
 *   bounds[6] = {min xyz, max xyz} (host values);  t_lin_c[Sc]: th.linspace(0, 1, Sc) (device; computed by the caller so that it is
 *         bit-identical to torch's)
 *   outputs, R = n_views*nx*ny: index[R] (int64 pixel index x + y*W), rays_d[R][3], cam_pos (device: [3] with a by-value camera,
 *            [n_views][4] with a table), near[R], far[R], hit[R] (u8),
 *            z[R][Sc] coarse depths (uniform=True: t_lin_c; else stratified with jitter[R][Sc] in [0,1) drawn by the caller) */
struct VanerfPassDesc;
int vanerf_ray_setup(const struct VanerfPassDesc* desc, int64_t* index, float* rays_d, float* cam_pos, float* near, float* far, uint8_t* hit,
                     float* z, void* stream);

/* eval_pts = cam_pos + dir * z (src/model.py:1234-1235).  pts[R*S][3].  rays_per_view = 0: one origin cam_pos[3]; > 0: ray r starts at
 * cam_pos[r / rays_per_view][4] (the table vanerf_ray_setup writes from a camera table), and R is a whole number of views. */
int vanerf_sample_points(const float* rays_d, const float* cam_pos, const float* z, int R, int rays_per_view, int S, float* pts, void* stream);

/* a6  get_visibility (mesh_util.py:284-318): vert_xy01[NV][2], vert_z01[NV], faces[NF][3] int32 -> vert_vis[NV];
 *     pix_to_face[S*S] int32 is scratch (may be NULL only if `scratch` given).                                          */
int vanerf_vertex_visibility(const float* vert_xy01, const float* vert_z01, int nv, const int32_t* faces, int nf,
                             int raster, int32_t* pix_to_face, float* vert_vis, void* stream);

/* a6  cal_vis_sdf_batch (mesh_util.py:498-524): signed distance, closest face, interpolated visibility.
 *     verts[NV][3], faces[NF][3] int32, vert_vis[NV], pts[N][3] -> sdf[N], vis[N] (u8), face[N] (int32, may be NULL)     */
int vanerf_mesh_query(const float* verts, int nv, const int32_t* faces, int nf, const float* vert_vis,
                      const float* pts, int64_t n, float* sdf, uint8_t* vis, int32_t* face, void* stream);

/* Acceleration structure for vanerf_mesh_query_accel, built per source frame by vanerf_mesh_accel_build below.
 * Results are bit-identical to vanerf_mesh_query.  Tested (tests/test_mesh_geometry.py, also against an fp64 definition of distance,
 * sign, arg-min face, visibility and 1-NN) on closed meshes in metres within a few metres of the origin -- |coordinate| up to 3.3 for the
 * hand meshes, 7 for ray samples about a 1 m torus -- at 0.5x, 1x and 2x the scale of a hand: star-shaped blobs, lobed (concave) hands of
 * 779 to 2 402 vertices, two interpenetrating hands, a torus, a sphere with a cavity, and cell grids of 1 to 256 cells a side.          */
/* Triangles / vertices per cluster the library was built with. */
int vanerf_mesh_cluster_size(void);

typedef struct {
    const float* tri;          /* [nfp][9]  triangle corners, Morton-sorted, padded to a multiple of the cluster size with far-away triangles */
    const float* sphere;       /* [nfp][4]  bounding sphere of each triangle (centroid, radius) */
    const float* tnorm;        /* [nfp][4]  unit normal of each triangle (0 for a degenerate one), w = rounding allowance 1e5 a^2: with `sphere` the triangle lies in the
                                *           disc {centroid + u : u normal to tnorm, |u| <= radius} -- the lower bound the search prunes with */
    const int32_t* orig;       /* [nfp]     original face index (INT32_MAX for padding) */
    const float* cbox;         /* [nc][6]   AABB of each cluster of vanerf_mesh_cluster_size() consecutive triangles (lo xyz, hi xyz) */
    int nfp, nc;
    const int32_t* cell_start; /* [G*G + 1] CSR offsets of the (y,z) grid used by the inside test */
    const int32_t* cell_tri;   /* original face ids per cell */
    const float* cell_rec;     /* [entries][12] the same lists as self-contained records: vertex ids i0 i1 i2 (int bits), corners a b c -- one load per entry in the inside test */
    const float* grid;         /* [5] DEVICE record of that grid: y0, z0, cell size in y, in z, G as int bits.  cell = clamp(floor((c - c0) / size), 0, G-1) */
    const float* vsort;        /* [nvc*CL][4] Morton-sorted vertices (xyz, original index as int bits), padded with far points */
    const float* vbox;         /* [nvc][6]    AABB of each cluster of CL vertices */
    int nvc;
    const float* cdisc;        /* [nc][8]  cylinder around each triangle cluster: (centre xyz, radius), (unit axis xyz, half height); the axis may be 0
                                *           (then radius alone bounds the distance from the centre: a ball).  Every vertex of the cluster's triangles
                                *           lies inside; second lower bound of the tile search of vanerf_mesh_query_accel (ray-grid hint) */
} VanerfMeshAccel;

/* Builds the tables above on the device, on `stream`, without a host synchronisation (seven small launches;
 * no counterpart in the reference: kaolin's point_to_mesh_distance / check_sign behind cal_vis_sdf_batch, src/lib/dataset/mesh_util.py:498-524, and
 * pytorch3d's knn_points, src/networks.py:28, scan all faces / vertices per point -- this is what lets vanerf_mesh_query_accel give their answers without; 0.1 ms for the two-hand MANO mesh):
 *     verts[NV][3], faces[NF][3] int32 (indices inside [0, NV): the caller's responsibility) -> *out, whose pointers point into `tables`,
 *     a caller-owned 16-byte-aligned device block of at least vanerf_mesh_accel_bytes(nv, nf, G, cell_capacity) bytes that must stay alive
 *     (and unmodified) for as long as *out is used.  G x G = cells of the (y,z) grid of the inside test (1..256; 64 for a hand mesh);
 *     cell_capacity >= nf = entries of the cells' triangle lists (64 * nf is ample: at G = 64 a triangle of a hand mesh touches ~20 cells).  Lists
 *     that would not fit make the grid degrade, on the device, to ONE cell listing every triangle: slower inside test, same results.
 *     Meshes of up to 16 384 faces / 4 096 vertices (the LDS-resident tables of vanerf_mesh_query_accel).                                  */
int64_t vanerf_mesh_accel_bytes(int nv, int nf, int G, int cell_capacity);   /* < 0: error code */
int vanerf_mesh_accel_build(const float* verts, int nv, const int32_t* faces, int nf, int G, int cell_capacity, void* tables,
                            int64_t tables_bytes, VanerfMeshAccel* out, void* stream);

/* knn_idx (may be NULL): 1-NN vertex of every point (knn_points K=1, src/networks.py:28), found in the same pass.
 * grid_nx, grid_ny, grid_s: optional layout hint (0,0,0 = none): pts are the samples of a grid_nx x grid_ny ray grid with grid_s
 * samples per ray in the reference's order (sample index = ray * grid_s + depth); lets a wave work on 64 neighbouring points.
 * The results do not depend on the hint.                                                                                      */
/* queue_word: 8 bytes of device memory owned by the caller for the duration of the launch (8-byte aligned; any contents): the head of the
 * kernel's work queue.  The library zeroes it on `stream` ahead of the launch and keeps NO device-side state of its own, so any number
 * of launches may be in flight on any number of streams as long as each has its own word (vanerf_render_pass takes them from its scratch). */
int vanerf_mesh_query_accel(const VanerfMeshAccel* accel, const float* verts, int nv, const int32_t* faces, int nf,
                            const float* vert_vis, const float* pts, int64_t n, float* sdf, uint8_t* vis, int32_t* face,
                            int32_t* knn_idx, int grid_nx, int grid_ny, int grid_s, void* queue_word, void* stream);

/* The same query with an item order on top of the ray-grid hint (which it needs).  By the hint alone a wave takes depth k of an 8 x 8 pixel
 * tile -- 64 neighbouring points only where the 64 rays put their k-th sample at one depth.  Importance samples and rays with different clip
 * ranges (the silhouette of the bounding box) do not; their tiles are searched over a needlessly wide range.
 *     item_order[ntx * nty * 64 * grid_s] (ntx = ceil(grid_nx / 8), nty = ceil(grid_ny / 8)), tile after tile, or NULL: lane l of depth k of a
 *         tile then works on sample item_order[(tile * grid_s + k) * 64 + l]; a slot that holds -1 names no sample.  Every sample index of
 *         [0, n) has to appear once (anywhere in the table: the kernel does not assume that it is sorted, nor that a tile names its own rays).
 *         Inputs are read and outputs written at the sample's own index either way: the results do not depend on `item_order`, only the
 *         time does.  NULL is vanerf_mesh_query_accel.
 * vanerf_mesh_tile_order writes the table the pass uses: z[grid_nx * grid_ny][grid_s] are the depths the points were made from; every tile's
 * sample indices in ascending z, equal depths in index order (for finite z exactly a stable sort of the tile's depths; with a NaN in a tile,
 * some permutation of that tile), the slots of rays beyond the grid border at the end of their tile, -1.  One launch, one block per tile,
 * sorted in LDS, no atomics (the same table on every run).  grid_s <= 128, more is refused.                                              */
int vanerf_mesh_query_accel_ordered(const VanerfMeshAccel* accel, const float* verts, int nv, const int32_t* faces, int nf,
                                    const float* vert_vis, const float* pts, int64_t n, float* sdf, uint8_t* vis, int32_t* face,
                                    int32_t* knn_idx, int grid_nx, int grid_ny, int grid_s, void* queue_word, const int32_t* item_order,
                                    void* stream);
int vanerf_mesh_tile_order(const float* z, int grid_nx, int grid_ny, int grid_s, int32_t* order, void* stream);

/* a10 knn_points K=1 (src/networks.py:28): verts[NV][4], pts[N][3] -> idx[N] int32 (first minimum). */
int vanerf_knn1(const float* verts4, int nv, const float* pts, int64_t n, int32_t* idx, void* stream);

/* a7-a15  VANeRF.query + eval_func for N samples (src/model.py:748-957, 1140-1160), n_views = 1:
 *     pts[N][3], query_sdf[N], query_vis[N] (u8), knn_idx[N] (1-NN vertex, from vanerf_mesh_query_accel or vanerf_knn1),
 *     noise[N] or NULL (rand_noise_std draws, model.py:1156)
 *     order[N] or NULL: a permutation of 0..N-1 from vanerf_query_order; slot k of the launch then works on sample order[k].  Inputs are
 *         read and outputs written at the sample's own index either way: the results do not depend on `order`, only the time does.
 *     raw = 0 -> out[N][5] = [alpha, sdf, r, g, b] (eval_func applied);  raw = 1 -> [sdf_pred, rad, r, g, b] as VANeRF.query returns
 *     valid[N] (u8, may be NULL)
 *     vertex_products: the frame's table from vanerf_vertex_products below (built with the same handle, after its last update), or NULL.  With the
 *         table a bf16x3 handle runs the lean kernel on its lean stream (which = 4 above): it starts the three layers' accumulators from the
 *         gathered table rows and runs their per-sample k-steps only, reads the two folded layers' products from the packed weights and starts
 *         five more accumulators from the bias table (outputs within 2e-5 of the un-hoisted kernel's: summation order).  The environment
 *         variable VANERF_LEAN_STREAM=0, read at every launch, selects the hoisted kernel on the hoisted stream instead (the lean kernel's
 *         predecessor, for A/B runs).  NULL selects the un-hoisted kernel.
 *         Where the frame's 64-channel geometry map has at most 1024 texels (h0 * w0; 32 x 32 for a 256 x 256 source) the table also holds the
 *         per-texel products of that map and the launch runs the texel kernel on the handle's texel stream (the library's stream 8, with a
 *         copy of the bias table, 9, behind it; 7 is no stream; neither has a name in the enum above): the lean kernel with the pixel
 *         feature's share of geo_vis_fusion.fconv_at.0 / fconv_ated.0 sampled from the table instead of multiplied per sample (outputs
 *         within 2e-5 of the lean kernel's: summation order).  A larger map runs the lean kernel.  VANERF_TEXEL_PRODUCTS=0, read at every
 *         launch, selects the lean kernel as well (its bits are what they were).                                                            */
int vanerf_query_samples(const VanerfWeights* w, const VanerfFrame* frame, const float* pts, const float* query_sdf,
                         const uint8_t* query_vis, const int32_t* knn_idx, const float* noise, const int32_t* order, int raw, int64_t n,
                         float* out, uint8_t* valid, void* queue_word /* as for vanerf_mesh_query_accel */, const float* vertex_products,
                         void* stream);

/* The per-vertex half of three first layers, once per source frame (bf16x3 handles).  geo_vis_fusion.fconv_at.0, geo_vis_fusion.fconv_ated.0 and
 * tex_vis_fusion.fconv_at.0 (src/networks.py:86-93, 285-288) multiply, per sample, rows of the frame's vertex tables that depend only on the
 * sample's 1-NN vertex; their products are a fixed vector per vertex: table = [A0 | N0 | T0 | P] (vanerf_amd/csrc/layer_spec.h), fp32, evaluated in
 * fp32 in a fixed order (two builds give the same bits).  table == NULL: returns the number of floats needed (> 0).  Otherwise one launch on
 * `stream` into table[cap_floats] (16-byte aligned; no allocation, no host synchronisation), returns 0; < 0: error.  The table belongs to
 * (handle contents, frame): rebuild it after vanerf_weights_update -- the library keeps no cache.
 * Behind P the table has room for the per-texel products of frame->geo0 with the pixel columns of the two geo layers, [GA | GM], 1024 texels
 * of 16 + 64 floats (a second launch on `stream`; 1.5 MB + 320 KB in all -- size the table by the NULL call, never by a constant).  A frame
 * with h0 * w0 > 1024 leaves that part unwritten, and vanerf_query_samples / vanerf_render_pass then run the lean kernel for it.          */
int vanerf_vertex_products(const VanerfWeights* w, const VanerfFrame* frame, float* table, int64_t cap_floats, void* stream);

/* Validity partition for vanerf_query_samples: order[N] = the samples whose projection hits the source view and its foreground mask
 * (src/model.py:780-803), in their order, then the others, in their order.  A 32-sample group of vanerf_query_samples in which no sample
 * is valid skips the geometry networks; with this order only one group per launch is mixed.  scratch: device memory of at least
 * vanerf_query_order_scratch(n) bytes.                                                                                          */
int vanerf_query_order(const VanerfFrame* frame, const float* pts, int64_t n, int32_t* order, void* scratch, int64_t scratch_bytes,
                       void* stream);
int64_t vanerf_query_order_scratch(int64_t n);

/* a16  sdf_activation + rgba2out (src/model.py:879-882, 1464-1494), with S = Sa samples per ray of one table (rgba_n == NULL; mesh_sdf_n, Sn, src ignored):
 *     rgba[R][S][5], z[R][S], mesh_sdf[R][S] -> color[R][3], depth[R], alpha[R], sdf[R], contrib[R][S] (may be NULL)
 * a16 + a18  or, with a second table, the fine composite that re-uses the coarse evaluations: S = Sa + Sn, sample i of ray r is entry src[r][i] (>= 0)
 *     of rgba[R][Sa][5] / mesh_sdf[R][Sa] (the coarse samples) or entry ~src[r][i] (< 0) of rgba_n[R][Sn][5] / mesh_sdf_n[R][Sn] (the importance
 *     samples), in the merged depth order z[R][Sa+Sn] produced by vanerf_importance_merge.  Identical bits to the one-table form on a
 *     re-evaluated (R, Sa+Sn) batch (the networks are per-sample pure functions).
 * beta: sigmoid_beta by value (> 0; clamped to >= 2e-3).  vanerf_composite_handle is the same call with sigmoid_beta read from the weight handle's
 * device copy instead (what vanerf_render_pass does; after vanerf_weights_update the host never sees the value).                               */
int vanerf_composite(const float* rgba, const float* z, const float* mesh_sdf, int Sa, const float* rgba_n, const float* mesh_sdf_n, int Sn,
                     const int32_t* src, int R, float beta, float* color, float* depth, float* alpha, float* sdf, float* contrib, void* stream);
int vanerf_composite_handle(const VanerfWeights* w, const float* rgba, const float* z, const float* mesh_sdf, int Sa, const float* rgba_n,
                            const float* mesh_sdf_n, int Sn, const int32_t* src, int R, float* color, float* depth, float* alpha, float* sdf,
                            float* contrib, void* stream);
/* eval_func (src/model.py:1140-1160) on raw outputs of vanerf_query_samples(raw = 1): [sdf_pred, rad, r, g, b] -> [alpha, sdf, r, g, b] with the validity
 * flags and optional per-sample noise, the arithmetic of the kernel's own epilogue (same bits).  src == NULL: R x Sa entries of table a, noise[i] per entry;
 * otherwise noise[r][p] belongs to position p of ray r's merged order and src names the entry (>= 0 table a, < 0 entry ~src of table b), each written once.
 * The outputs may be the raw tables themselves (rgba_a == raw_a, rgba_b == raw_b: every entry is read, then written, by one thread).  With training noise a pass evaluates the networks once per point and runs this once per set of draws.     */
int vanerf_eval_func(const float* raw_a, const uint8_t* valid_a, const float* raw_b, const uint8_t* valid_b, const int32_t* src, const float* noise,
                     int Sa, int Sb, int R, float invalid_sdf, float* rgba_a, float* rgba_b, void* stream);
/* Training: the backward of either composite (reference: autograd through rgba2out / sdf_activation, src/model.py:1464-1494, 879-882), tables and src as
 * vanerf_composite_handle.  g_color [R][3], g_depth, g_alpha, g_sdf [R]: gradients with respect to the composite's outputs (any may be NULL = 0);
 * d_rgba [R][Sa][5] (and d_rgba_n [R][Sn][5]): gradient with respect to every table entry (each is written once), d_beta [R] or NULL: the rays' shares
 * of the gradient with respect to the (clamped) sigmoid_beta.  At most 256 samples per ray.                                                            */
int vanerf_composite_backward(const VanerfWeights* w, const float* rgba, const float* z, const float* mesh_sdf, int Sa, const float* rgba_n,
                              const float* mesh_sdf_n, int Sn, const int32_t* src, int R, const float* g_color, const float* g_depth,
                              const float* g_alpha, const float* g_sdf, float* d_rgba, float* d_rgba_n, float* d_beta, void* stream);

/* a17  importance_sample + sort-merge (src/model.py:1424-1462, 1301-1307):
 *     contrib[R][Sc], z[R][Sc], u[R][Sf] (random draws) or NULL with t_lin[Sf] = th.linspace(0, 1, Sf) (uniform=True) ->
 *     z_new[R][Sf], z_fine[R][Sc+Sf] (sorted), src[R][Sc+Sf] int32 (>= 0: coarse sample id, < 0: ~(new sample id)),
 *     idx[R][Sf] int32 searchsorted index after clamping (may be NULL)                                                   */
int vanerf_importance_merge(const float* contrib, const float* z, const float* u, const float* t_lin, int R, int Sc, int Sf,
                            float* z_new, float* z_fine, int32_t* src, int32_t* idx, void* stream);

/* a17 in the reference's own call shape (src/model.py:1304, 1424-1462): contrib_inner[R][n_bins] = contrib[..., 1:-1],
 *     z_mid[R][n_bins+1] -> z_new[R][Sf]; idx[R][Sf] (searchsorted index after clamping, may be NULL).                     */
int vanerf_importance_sample(const float* contrib_inner, const float* z_mid, const float* u, const float* t_lin, int R, int n_bins,
                             int Sf, float* z_new, int32_t* idx, void* stream);

/* One whole pass -- VANeRF.batch_render_pifu_nerf without its GT-gather tail (src/model.py:1102-1360): rays, bbox clip, coarse depths,
 * mesh queries, validity partition, per-sample networks, composite, importance sampling + merge, fine march, fine composite -- as ONE call that
 * enqueues the kernels above on `stream` in the order vanerf_amd/renderer.py:render_pass does (same kernels, same arguments: same bits).
 * No allocation, no host synchronisation: all temporaries live in `scratch` (device memory of at least vanerf_render_pass_scratch(...) bytes,
 * caller-owned; two passes may run concurrently on different streams with different scratch blocks and the same weights handle).            */
typedef struct VanerfPassDesc {
    int x0, y0, step_x, step_y, y_block, nx, ny; /* pixel grid as in vanerf_ray_setup (ignored when pixels_xy is given; then nx * ny rays are listed) */
    const int32_t* pixels_xy;  /* optional explicit pixel list [nx*ny][2] (device) */
    const int32_t* row_blocks; /* optional first rows of the ny / y_block blocks of rows (device); y0, step_y ignored */
    int width;                 /* target image width (pixel index = x + y * width) */
    int n_views;               /* >= 1 target views of the one source frame that share the grid and width; must be 1 when cams == NULL */
    const float* cams;         /* NULL: the camera is invK_T / RT / znear / zfar below.  Else the [n_views][24] DEVICE table invK_T[9], RT[12], znear,
                                  zfar, pad per view, and the by-value camera is not read.  The table form is the evaluation form: it takes the plain
                                  grid only (no pixels_xy, no row_blocks, y_block = 1) and no noise_c / noise_f */
    float invK_T[9], RT[12];   /* target camera: inverse(K[:3,:3]) transposed; [R|t] rows 0..2 */
    float znear, zfar;
    float bounds[6];           /* {min xyz, max xyz} of the mesh bounding box (config['bounds']) */
    int Sc, Sf;                /* sample_per_ray_c, sample_per_ray_f */
    int fine;                  /* config['fine'] */
    int reuse_coarse;          /* 1: the fine composite re-uses the coarse evaluations (only the Sf new samples are evaluated; identical bits).  With
                                  noise_c / noise_f (training) the networks still run once per point: raw outputs, then eval_func with the coarse draws
                                  and again with the fine batch's draws (vanerf_eval_func) -- the noise is added to the networks' OUTPUT
                                  (src/model.py:1155-1156), so the bits are those of re-evaluating all Sc + Sf samples */
    const float* t_lin_c;      /* th.linspace(0, 1, Sc) (device) */
    const float* t_lin_f;      /* th.linspace(0, 1, Sf) (device); used when u == NULL (uniform=True) */
    const float* jitter;       /* [R][Sc] stratification draws or NULL (uniform=True); R = n_views * nx * ny, view-major */
    const float* u;            /* [R][Sf] importance draws or NULL */
    const float* noise_c;      /* [R*Sc] rand_noise_std * randn draws for the coarse march, or NULL */
    const float* noise_f;      /* [R*(Sc+Sf)] the same for the fine march (required with noise_c when fine) */
} VanerfPassDesc;

typedef struct {               /* all device pointers; R = n_views * nx * ny, view-major */
    int64_t* index;            /* [R]    pixel index */
    uint8_t* hit;              /* [R]    ray crosses the bounding box */
    float* z;                  /* [R][Sc] coarse depths */
    float* color;              /* [R][3] coarse colour   (tex_fg)   */
    float* depth;              /* [R]                    (depth)    */
    float* alpha;              /* [R]                    (alpha)    */
    float* color_fine;         /* [R][3] (tex_fg_fine); the four fine outputs may be NULL when fine == 0 */
    float* depth_fine;         /* [R] */
    float* alpha_fine;         /* [R] */
    float* sdf;                /* [R] */
    float* z_fine;             /* [R][Sc+Sf] merged depths, or NULL */
} VanerfPassOut;

/* Bytes of scratch a pass over n_views views of rays_per_view = nx * ny rays needs.  reuse_coarse: 0, 1 as VanerfPassDesc.reuse_coarse; 2 = re-use
 * under per-sample noise (desc->reuse_coarse with noise_c given: more temporaries).  0: bad arguments, or the largest march of the pass,
 * n_views * nx * ny * (Sc, max(Sc, Sf) with re-use, or Sc + Sf), reaches 2^31 - 1: the 32-bit sample index of vanerf_query_order bounds every
 * pass (a single view that large used to fail inside vanerf_query_order; now here and at the head of vanerf_render_pass). */
int64_t vanerf_render_pass_scratch(int n_views, int rays_per_view, int Sc, int Sf, int fine, int reuse_coarse);
/* With a camera table the kernels run once over n_views * nx * ny rays instead of n_views times over nx * ny (the frames of an orbit, the views
 * of a validation step): behind the ray setup nothing depends on the camera but the ray origin, so view v's slice of every output holds the
 * bits the by-value form gives for that camera alone.
 * vertex_products: the frame's table of vanerf_vertex_products for the pass's per-sample launches, or NULL (as vanerf_query_samples) */
int vanerf_render_pass(const VanerfWeights* w, const VanerfFrame* frame, const VanerfMeshAccel* accel, const float* verts, int nv,
                       const int32_t* faces, int nf, const VanerfPassDesc* desc, const VanerfPassOut* out, void* scratch, int64_t scratch_bytes,
                       const float* vertex_products, void* stream);

/* Training step, backward of the row gathers (bilinear taps of feat_sample, src/utils.py:136-151; nearest / twin vertex rows of KNN_vis,
 * src/networks.py:27-33):  table[idx[i]][0..C) += w[i] * g[i][0..C)  for i < n  (w may be NULL = 1; rows outside [0, R) are ignored).
 * All device pointers, fp32 / int32; `table` is accumulated into.  Samples outnumber rows by hundreds: the adds go through LDS-resident
 * slices of the table instead of contended global atomics.                                                                               */
/* g_ld: floats between consecutive rows of g (0 = C: packed rows).                                                                        */
int vanerf_scatter_add_rows(const int32_t* idx, const float* w, const float* g, int64_t g_ld, int64_t n, int C, float* table, int R, void* stream);
/* the four bilinear taps of feat_sample (src/utils.py:136-151; border padding, align_corners) at xy[n][2] in [-1, 1] on an H x W map: idx4 / w4 = [4][n], the
 * row indices of the channel-last map and the weights vanerf_scatter_add_taps takes                                                              */
int vanerf_bilinear_taps(const float* xy, int64_t n, int H, int W, int32_t* idx4, float* w4, void* stream);
/* two sources into one table in one launch (the nearest and the twin vertex row of a sample): table[idx[i]] += w[i] g[i], table[idx2[i]] += w2[i] g2[i] */
int vanerf_scatter_add_rows2(const int32_t* idx, const float* w, const float* g, const int32_t* idx2, const float* w2, const float* g2, int64_t g_ld,
                             int64_t n, int C, float* table, int R, void* stream);
/* the same with FOUR (index, weight) pairs per sample, idx4 / w4 = [4][ld] (ld >= n): the backward of a bilinear tap gather (src/utils.py:136-151) */
int vanerf_scatter_add_taps(const int32_t* idx4, const float* w4, int64_t ld, const float* g, int64_t g_ld, int64_t n, int C, float* table, int R,
                            void* stream);

/* f-4, the fused backward pass of the per-sample networks (training; reference: autograd through VANeRF.query, src/model.py:748-957, driven by
 * training_step, src/model.py:381-459).  Two launches per block of n samples, on one stream, with an fp32 weight handle (vanerf_weights_pack mode 0):
 *   vanerf_query_forward_spill  the forward pass once more (raw outputs [sdf_pred, rad, r, g, b], validity), which also writes every layer's operands
 *                               X and the gates / pixel weight / pre-pooling latent the backward needs:  xs[x_rows][npad], aux[aux_rows][npad]
 *   vanerf_query_backward       d[n][5]: gradient with respect to eval_func's outputs [alpha, sdf, r, g, b] (src/model.py:1140-1160; d2 / noise /
 *                               noise2 may be NULL: a second set of draws on the same points, the density noise) with raw / valid of the spill pass
 *                               -> ys[y_rows][npad]: every layer's output gradient, and
 *                               ig[ig_rows * npad]: the gradients of the gathered inputs (pixel taps, nearest / twin vertex rows) as nine ROW-MAJOR
 *                               tensors [npad][stride] one after the other (vanerf_ig_tensor), which vanerf_scatter_add_rows / _taps read as they stand
 * xs, aux, ys: channel-major fp32 spills, npad = n rounded up to a multiple of 32 (columns >= n carry zero gradients); row counts: vanerf_spill_rows.
 * The weight gradient of layer l is then one matrix product over the samples, dW'[out][slot] = ys_l xs_l^T with the rows of
 * vanerf_layer_rows and the slot -> input-channel table of vanerf_layer_slots (slot 2 t + h; -1 unused, -2 bias: that column is the bias
 * gradient); vanerf_amd/hip_backward.py does this with torch.bmm and hands ig to vanerf_scatter_add_rows.                                */
int vanerf_query_forward_spill(const VanerfWeights* w, const VanerfFrame* frame, const float* pts, const float* query_sdf,
                               const uint8_t* query_vis, const int32_t* knn_idx, int64_t n, int64_t npad, float* out_raw, uint8_t* valid,
                               float* xs, float* aux, void* queue_word, void* stream);
int vanerf_query_backward(const VanerfWeights* w, const float* d, const float* d2, const float* noise, const float* noise2, const float* raw,
                          const uint8_t* valid, int64_t n, int64_t npad, const float* xs, const float* aux, float* ys, float* ig, void* stream);
int vanerf_spill_rows(int* x_rows, int* y_rows, int* aux_rows, int* ig_rows);
/* The weight gradients of a block: dw[slice][layer l at (sum of n_out x n_slots over the layers before l)][n_out][n_slots] += ys_l xs_l^T over the slice's
 * samples, every layer in one launch (slices: the block's samples are cut into this many parts that accumulate separately -- the caller sums dw over its
 * first dimension once per step; npad must be a multiple of 32 x slices; slices <= layout_slices, the number of parts dw has room for;
 * vanerf_weight_products_size: floats per part).  One wave per (tile group, slice): no atomics, reproducible.                                       */
int vanerf_weight_products(const float* xs, const float* ys, int64_t npad, int slices, int layout_slices, float* dw, void* stream);
int vanerf_weight_products_size(int64_t* floats_per_slice);
/* Tensor `which` of the ig spill: 0..2 pixel feature / nearest / twin vertex row of GeoVisFusion's scale 0 (64 channels), 3..5 the same of scale 1
 * (8), 6, 7 TexVisFusion's nearest / twin vertex row [img3 | tex8 | global18] (29 of 32), 8 the texture map's pixel feature (8).  The tensor
 * starts at ig + offset * npad, has `channels` channels and `stride` floats per row.  Returns the number of tensors (9), < 0: error.          */
int vanerf_ig_tensor(int which, int* offset, int* channels, int* stride);
int vanerf_layer_slots(int layer, int32_t* k_of_slot, int cap);              /* returns 2 T (k-pairs x lane halves), < 0: error */
int vanerf_layer_rows(int layer, int* x_row, int* y_row, int* n_out);

/* a3  ray_bbox_intersection (src/model.py:1496-1570) alone: bounds[6], orig[3] (host values), dirs[R][3] (device)
 *     -> near[R], far[R] (1.0 when the ray does not cross the box exactly twice), hit[R] (u8).                               */
int vanerf_ray_bbox(const float* bounds, const float* orig, const float* dirs, int R, float* near, float* far, uint8_t* hit, void* stream);

/* render_vis (src/render_vis.py:181-226): the mesh rendered in the target camera with the per-vertex visibility as its colour,
 * Phong-shaded and blended, and the visibility image thresholded from it.  Semantics restated from pytorch3d 0.7.5;
 * parity against pytorch3d itself is unpinned.
 *     verts[NV][3] (world, metres), faces[NF][3] int32 (a face with an index outside [0, NV) draws nothing), vert_vis[NV] ({0, 1}),
 *     R[3][3], T[3]: pytorch3d row-vector convention, Xv = X_world R + T;  focal[2] = (fx, fy), princpt[2] = (px, py): screen space,
 *         vertex -> (px - fx Xv/Zv, py - fy Yv/Zv); pixel (row r, col c) samples (c + 0.5, r + 0.5).  All four are DEVICE pointers.
 *     scratch: device memory of at least NV * 16 floats (16-byte aligned): per vertex (u, v, x_ndc, y_ndc), (Xv, Yv, Zv, vert_vis),
 *         (world xyz, 0), (unit vertex normal, 0) -- written by the vertex pass, read by the raster pass.
 *     -> rgb[3][H][W] (vis_img_rbg), vis[H][W] (vis_img: 1 where mean(rgb * 255) >= 50, else 0; the background is 1),
 *        pix_to_face[H][W] int32 (-1: background) and zbuf[H][W] (view depth, -1: background), both may be NULL.
 *     Two launches on `stream`; no allocation, no host synchronisation.                                                      */
int vanerf_render_vis(const float* verts, int nv, const int32_t* faces, int nf, const float* vert_vis, const float* R, const float* T,
                      const float* focal, const float* princpt, int H, int W, float* scratch, int64_t scratch_bytes, float* rgb, float* vis,
                      int32_t* pix_to_face, float* zbuf, void* stream);

/* Image scores of the reference's validation and test steps for V rendered views, on the device.  Neither kornia
 * nor scikit-image is a dependency: the arithmetic is restated below, parity against kornia 0.7.1 / scikit-image 0.16.2 is unpinned.
 *     pred[V][3][H][W], gt[V][3][H][W] fp32 (channel-first, as render_pifu_nerf returns them); clamp_pred != 0: pred is clamped to [0, 1]
 *     on load.  mask[V][H][W], mask_at_box[V][H][W]: uint8, nonzero = set, either may be NULL.  All are DEVICE pointers.
 *     -> out[V][8] fp32 (device):
 *        0 mse          mean of (pred - gt)^2 over the 3 H W elements                          (Evaluator.compute_score, src/evaluator.py:84-114)
 *        1 psnr         -10 log10(mse)
 *        2 ssim_box     skimage structural_similarity(multichannel=True) of float images on the crop to cv2.boundingRect(mask_at_box) (the
 *                       whole image without one): 7 x 7 uniform window, data_range 2 (C1 = 0.02^2, C2 = 0.06^2), sample covariance
 *                       v = 49/48 (E[xy] - E[x]E[y]), S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)) averaged over the
 *                       windows that lie wholly inside the crop, per channel, then over the channels.  NaN for an empty mask or a crop
 *                       narrower or lower than 7 (the reference raises there)
 *        3 psnr_masked  10 log10(max_val^2 / mean((pred - gt)^2)) over the pixels of mask x 3 channels    (compute_test_metric, src/model.py:210-235)
 *        4 ssim_masked  mean over the same elements of kornia's ssim(window_size=7): 7 x 7 Gaussian window (sigma 1.5, normalised outer
 *                       product of the 1-D kernel), images reflect-padded by 3 without repeating the edge pixel, sigma = E[x^2] - mu^2,
 *                       C1 = (0.01 max_val)^2, C2 = (0.03 max_val)^2, S = num / (den + 1e-12).  Without a mask every pixel counts;
 *                       slots 3 and 4 are NaN for an empty mask
 *        5 n_mask, 6 box_w, 7 box_h   (exact)
 *     scratch: vanerf_image_metrics_scratch(V, H, W) bytes of device memory, 16-byte aligned (0: not a valid shape; 1 <= V <= 65535,
 *         4 <= H, W <= 4096).  Every byte the call reads of it is written by the call first: its previous contents do not matter.
 *     Three launches on `stream`; no allocation, no host synchronisation, no atomics: the same bits every call, per view whatever V is.     */
int64_t vanerf_image_metrics_scratch(int V, int H, int W);
int vanerf_image_metrics(const float* pred, const float* gt, const uint8_t* mask, const uint8_t* mask_at_box, int V, int H, int W,
                         double max_val, int clamp_pred, void* scratch, int64_t scratch_bytes, float* out, void* stream);

/* The dataset's mask_at_box and near / far range of V target views, on the device: Dataset.get_mask_at_box ->
 * get_rays / get_near_far (src/dataset.py:122-129, 609-658) restated.
 *     cams[V][24]: the DEVICE table of VanerfPassDesc.cams (invK_T[9], RT[12]; znear, zfar and the pad are not read).  bounds[6]: HOST,
 *     min xyz then max xyz, read before the call returns.  Per pixel (r, c) of view v, in fp64 from the fp32 values:
 *        pc = (c, r, 1) . invK_T,  o = -R^T T,  d = (pc - T) . R - o;  o and d are each rounded to fp32 once, and a component of d with
 *        |d| < 1e-5 becomes +1e-5 (both in fp32; the sign is lost, as in the reference).
 *        b = bounds + (-0.01, +0.01).  For each of the six planes (min x, y, z, max x, y, z): t = (b - o) / d on the plane's axis,
 *        p = t d + o; the plane is hit iff all three coordinates of p lie in [b_min - 1e-6, b_max + 1e-6].
 *        mask = exactly two planes are hit; near / far = the smaller / larger of |p - o| / |d| over the two hits.
 *     -> mask[V][H][W] uint8 (0 / 1); near[V][H][W], far[V][H][W] fp32 (either may be NULL): the ray's values on mask pixels, NaN elsewhere;
 *        out[V][8] fp32: 0 near_min, 1 far_max (NaN for an empty mask: the reference raises there), 2 n_mask, 3-6 box_x, box_y, box_w, box_h
 *        (cv2.boundingRect of the mask; 0, 0, 0, 0 for an empty one), 7 zero.  Slots 2-6 are exact.  All DEVICE pointers.
 *     scratch: vanerf_mask_at_box_scratch(V, H, W) bytes of device memory, 16-byte aligned (0: not a valid shape; 1 <= V <= 65535,
 *         1 <= H, W <= 4096).  Every byte the call reads of it is written by the call first: its previous contents do not matter.
 *     Two launches on `stream`; no allocation, no host synchronisation, no atomics: the same bits every call, per view whatever V is.       */
int64_t vanerf_mask_at_box_scratch(int V, int H, int W);
int vanerf_mask_at_box(const float* cams, int V, int H, int W, const float bounds[6], uint8_t* mask, float* near, float* far, void* scratch,
                       int64_t scratch_bytes, float* out, void* stream);

/* The learned surface as a triangle mesh.  The network predicts a residual on the MANO signed distance: with
 * alpha = valid relu(rad) of eval_func (src/model.py:1140-1160) the composite turns f = alpha + mesh_sdf into a density (1480-1481), and the
 * hand is the zero level set of f.  Four calls: points of a regular grid, f from the outputs of the two queries on them, and marching
 * tetrahedra over the grid of scalars in two steps with one host read (the counts) between them.
 *
 * A grid is origin[3], spacing[3] (HOST, read before the call returns; finite, spacing > 0) and nx, ny, nz >= 2 points per axis with
 * 7 nx ny nz < 2^31; point (x, y, z) has the linear index (z ny + y) nx + x and the position fmaf(index, spacing, origin) per axis: one
 * rounding, the same expression in every call below.
 *
 *     vanerf_grid_points: pts[nz_out ny nx][3] (device) = the points of layers z0 ... z0 + nz_out - 1 (a slab of the grid; 0 <= z0,
 *         z0 + nz_out <= nz).  One launch.
 *     vanerf_field_values: f[n] = rgba[n][0] + mesh_sdf[n], with rgba[n][5] = [alpha, sdf, r, g, b] of a query with raw = 0 and mesh_sdf of
 *         the mesh query; rgb[n][3] = rgba[n][2..4] unless NULL.  A non-finite sum is stored as it is.  All device pointers.  One launch.
 *
 * Marching tetrahedra over f[nz][ny][nx] (device), indexed and welded:
 *     - a value counts as INSIDE iff f < iso; a non-finite f is read as +FLT_MAX (outside), so no NaN reaches an output;
 *     - corners of a cell carry the code dx | dy << 1 | dz << 2; the cell is split into the six tetrahedra (0, e_a, e_a + e_b, 7) around its main
 *       diagonal, one per order (a, b, c) of the axes.  The split is the same in every cell, so neighbours agree on the diagonals of their
 *       common face and the surface is watertight; a tetrahedron with 1 or 3 corners inside gives one triangle, with 2 gives two;
 *     - every grid point owns the seven edges towards the direction codes d = 1 ... 7 (+x, +y, +xy, +z, +xz, +yz, +xyz) that stay inside the
 *       grid.  An edge with exactly one end inside carries one vertex at a + t (b - a), t = (iso - f_a) / (f_b - f_a) in fp32, a the owning
 *       point (the end with the lower linear index); the result is clamped onto the edge, so a vertex lies on its grid edge exactly.
 *       colors = rgb_a + t (rgb_b - rgb_a) with the same t;
 *     - every triangle is wound so that its normal ((v1 - v0) x (v2 - v0)) points from inside to outside, towards growing f;
 *     - vertices are numbered in the order (brick of 8 x 8 x 8 points, point in the brick, direction code), triangles in the order (brick,
 *       cell in the brick, tetrahedron), by exclusive scans in a fixed order: no atomics, the same bits every call whatever scratch held.
 *     vanerf_surface_count: -> counts[2] int64 (DEVICE) = {n_vertices, n_triangles}; the scanned offsets stay in scratch.  Two launches.
 *     vanerf_surface_emit: with the same f, grid, iso and scratch, and n_verts / n_tris as read from counts: -> verts[n_verts][3],
 *         colors[n_verts][3] (NULL: none; needs rgb[nz ny nx][3]), tris[n_tris][3] int32.  cap_verts / cap_tris: what the buffers hold; less
 *         than the counts is an error, and nothing is written past them in any case.  n_verts = n_tris = 0 is a no-op.  One launch.
 *     scratch: vanerf_surface_scratch(nx, ny, nz) bytes of device memory, 16-byte aligned (0: not a valid grid).  Every byte the calls read of
 *         it is written by vanerf_surface_count first.
 * All work goes to `stream`; no allocation, no host synchronisation.                                                                      */
int vanerf_grid_points(const float origin[3], const float spacing[3], int nx, int ny, int nz, int z0, int nz_out, float* pts, void* stream);
int vanerf_field_values(const float* rgba, const float* mesh_sdf, int64_t n, float* f, float* rgb, void* stream);
int64_t vanerf_surface_scratch(int nx, int ny, int nz);
int vanerf_surface_count(const float* f, int nx, int ny, int nz, float iso, void* scratch, int64_t scratch_bytes, int64_t* counts, void* stream);
int vanerf_surface_emit(const float* f, const float* rgb, const float origin[3], const float spacing[3], int nx, int ny, int nz, float iso,
                        const void* scratch, int64_t scratch_bytes, int64_t n_verts, int64_t n_tris, float* verts, float* colors, int32_t* tris,
                        int64_t cap_verts, int64_t cap_tris, void* stream);

/* The learned surface along lines: sample f on n lines base[i] + t dir[i] (base[n][3], dir[n][3] fp32), bracket the
 * crossing of f = iso nearest to t = 0 on every line and refine it with further values of f.  surface.register_surface runs these calls on the
 * lines through the MANO vertices along their vertex normals and moves every vertex to its crossing.  All pointers are DEVICE pointers.
 *
 *     vanerf_vertex_normals: normals[nv][3] = the unit vertex normals of the mesh (verts[nv][3], faces[nf][3] int32) with the arithmetic of the
 *         vertex pass of vanerf_render_vis: the face normal cross(v2 - v1, v0 - v1) added once per corner that names the vertex, a face with an
 *         index outside [0, nv) left out; one wave per vertex, lane l summing faces l, l + 64, ... in ascending order, a fixed xor butterfly over
 *         the lanes, then x / max(|x|, 1e-6).  The bits are those of floats 12..14 of vanerf_render_vis's scratch record.  One launch.
 *     vanerf_line_points: pts[n K][3], line-major.  t_dev == NULL: t_k = fmaf((float)k, dt, t0), k = 0 ... K - 1 (t0 finite, dt finite and
 *         positive), and the point is fmaf(t_k, dir, base) per axis.  t_dev != NULL: K must be 1, t = t_dev[i] (t0 and dt are not read), and a
 *         non-finite t is read as 0: the point is the base, bit for bit.  1 <= K <= VANERF_LINE_MAX_SAMPLES, n >= 0 (n = 0: a no-op),
 *         n K < 2^31.  One launch.
 *     vanerf_line_bracket: f[n][K] (and rgb[n][K][3], or NULL) at the points of the first form, 2 <= K -> state[n][VANERF_LINE_STATE_FLOATS].
 *         - clean value g = isfinite(f) ? f : FLT_MAX; a sample is INSIDE iff g < iso (the extractor's rule, so f == iso is outside);
 *         - a pair (k, k + 1) is a crossing iff exactly one of its ends is inside; its weight is w = clamp((iso - g_k) / (g_k+1 - g_k), 0, 1)
 *           in fp32, clamp(x, lo, hi) = fminf(fmaxf(x, lo), hi), and its parameter tc = fmaf(w, dt, t_k);
 *         - the line's crossing is the pair with the smallest |tc|, a tie going to the smaller k;
 *         - the record (floats, by the VANERF_LS_* offsets below): ta, tb = t_k, t_k+1; ga, gb = g_k, g_k+1; rgb_a, rgb_b = the rgb of the
 *           two samples (zeros without rgb); found = 1; t_est = fmaf(w, tb - ta, ta); rgb_est = rgb_a + w (rgb_b - rgb_a), product and sum
 *           rounded separately; t_next = fmaf(clamp(w, 0.125, 0.875), tb - ta, ta): where f is to be evaluated next;
 *         - a line without a crossing: found = 0, t_est = t_next = NaN, zeros elsewhere.
 *         One wave per line, the samples over the lanes (K > 64 in rounds of 64); one launch.  state must be 16-byte aligned.
 *     vanerf_line_refine: f_new[n] (and rgb_new[n][3], or NULL: the colours of the record stay) = the field at every line's t_next.  On a found
 *         line, with g the clean value: if g is on the same side of iso as ga, (ta, ga, rgb_a) <- (t_next, g, rgb_new), otherwise (tb, gb, rgb_b)
 *         take them; then w, t_est, rgb_est and t_next are recomputed with the expressions above.  Other lines are left as they are.  The bracket
 *         always has exactly one end inside, and it shrinks to at most 7/8 of its width per call (up to the rounding of t_next).  One launch.
 *     vanerf_line_state_floats: VANERF_LINE_STATE_FLOATS, for a binding that does not read this header.
 * All work goes to `stream`; no allocation, no host synchronisation, no atomics: every record is a function of its own line, the same bits
 * every call whatever state held.  Arguments are checked before any launch.                                                                */
#define VANERF_LINE_MAX_SAMPLES 256
#define VANERF_LINE_STATE_FLOATS 16
#define VANERF_LS_TA 0
#define VANERF_LS_TB 1
#define VANERF_LS_GA 2
#define VANERF_LS_GB 3
#define VANERF_LS_RGB_A 4   /* 4..6 */
#define VANERF_LS_FOUND 7   /* 1.0f or 0.0f */
#define VANERF_LS_RGB_B 8   /* 8..10 */
#define VANERF_LS_T_EST 11
#define VANERF_LS_RGB_EST 12 /* 12..14 */
#define VANERF_LS_T_NEXT 15
int vanerf_line_state_floats(void);
int vanerf_vertex_normals(const float* verts, int nv, const int32_t* faces, int nf, float* normals, void* stream);
int vanerf_line_points(const float* base, const float* dir, int n, int K, float t0, float dt, const float* t_dev, float* pts, void* stream);
int vanerf_line_bracket(const float* f, const float* rgb, int n, int K, float t0, float dt, float iso, float* state, void* stream);
int vanerf_line_refine(const float* f_new, const float* rgb_new, int n, float iso, float* state, void* stream);

/* The learned field baked into a voxel grid, and views rendered from it.  At one source view the colour of a sample does
 * not depend on the viewing direction, the density is a function of f = alpha + mesh_sdf alone and `valid` depends on the source camera only,
 * so (f, r, g, b) on a regular grid -- what vanerf_grid_points ... vanerf_field_values produce -- serves every camera of an orbit.  Rendering
 * from it is an APPROXIMATION of the pass (a grid resolution and uniform samples in place of the networks at 64 + 64 importance samples).
 * The grid is the one described above: origin[3], spacing[3] (HOST), nx, ny, nz >= 2, 7 nx ny nz < 2^31, x fastest.
 *
 *     vanerf_volume_pack: f[n], rgb[n][3] -> voxels[n][4] = (f, r, g, b), so a corner of a cell is one 16-byte load.  A non-finite f is stored as
 *         +1e30f: it reads as outside (sigmoid(-1e30 / beta) is exactly 0) and is finite, so eight weights that sum to 1 neither overflow nor
 *         meet 0 * inf.  A non-finite colour channel is stored as 0.  Everything else is copied bit for bit.  0 <= n < 2^31 (0: a no-op);
 *         voxels 16-byte aligned.  One launch.
 *     vanerf_volume_render: the rays vanerf_ray_setup writes for V views -- rays_d[R][3], cam_pos[V][4], z[R][S], hit[R], R = V rays_per_view
 *         rays, view-major; row_rays: the rays of one pixel row of a view (rays_per_view is a whole number of rows; it only decides which rays
 *         share a block) -> color[R][3], depth[R], alpha[R].  sigmoid_beta: from the handle w's device copy (already clamped at 2e-3), or, with
 *         w == NULL, `beta` by value (finite, > 0; clamped at 2e-3).  Per ray:
 *         - hit == 0: colour, depth and alpha are 0 and nothing else happens;
 *         - sample i is at p = o + d z_i per axis (vanerf_sample_points' expression); its grid coordinate per axis is u = (p - origin) / spacing,
 *           clamped to [0, n - 1] (border padding; a NaN clamps to 0), its cell i0 = min((int)floorf(u), n - 2) and its weight w = u - i0;
 *         - the four channels are interpolated from the eight corners in fp32, (1 - w) a + w b along x, then y, then z;
 *         - the composite is vanerf_composite's with a = the interpolated f in the place of rgba[0] + mesh_sdf:
 *           sg = (1 / (1 + expf(a / beta))) / beta, dist = z_i+1 - z_i (1e10f for the last sample), c = 1 - expf(-sg dist), w_i = c T,
 *           T *= 1 - c; colour, alpha and the z-weighted sum are accumulated in fp64 from fp32 products, depth = sum / (alpha + 1e-8f).
 *         One wave per ray, the samples over the lanes in rounds of 64 with the transmittance carried between rounds (an exclusive prefix
 *         product with a fixed shuffle pattern inside a round, a fixed xor butterfly for the sums), the waves of a block on a 2 x 2 pixel tile
 *         of one view.  Any S >= 1; V <= 65535; R == 0 is a no-op.  One launch.
 * All pointers but origin and spacing are DEVICE pointers.  All work goes to `stream`; no allocation, no host synchronisation, no atomics, no
 * device-side state: the same bits every call.  Arguments are checked before any launch.                                                 */
int vanerf_volume_pack(const float* f, const float* rgb, int64_t n, float* voxels, void* stream);
int vanerf_volume_render(const float* voxels, const float origin[3], const float spacing[3], int nx, int ny, int nz, const VanerfWeights* w, float beta,
                         const float* rays_d, const float* cam_pos, const float* z, const uint8_t* hit, int R, int rays_per_view, int row_rays, int S,
                         float* color, float* depth, float* alpha, void* stream);

/* The surface of the baked volume as a camera sees it: depth, normal and colour maps from the voxels of
 * vanerf_volume_pack and the rays of vanerf_ray_setup, with no network, no mesh query and no triangle.  The grid, the rays, their layouts and
 * row_rays are vanerf_volume_render's; voxels and normal 16-byte aligned; iso finite; 0 <= refine <= 4; any S >= 1; V <= 65535; R == 0 is a
 * no-op.  -> depth[R], normal[R][4] = (nx, ny, nz, n . v), color[R][3], found[R] (0, 1 or 2).  Per ray, all in fp32:
 *     - hit == 0: found = 0 and every output is 0.
 *     - g(zz) is channel 0 of vanerf_volume_render's trilinear interpolation at p = o + d zz (the same u, clamp, cell and (1 - w) a + w b order
 *       along x, then y, then z).  A point is INSIDE iff g < iso (vanerf_surface_count's rule: g == iso is outside).
 *     - sample 0 inside: found = 2 and z* = z_0 (the clipped ray starts inside the hand, as at the wrist, which the box cuts).  With S == 1 this
 *       is the only way to be found.
 *     - otherwise the smallest k with sample k outside and sample k + 1 inside: found = 1 and the bracket is (za, zb, ga, gb) =
 *       (z_k, z_k+1, g_k, g_k+1).  None: found = 0 and every output is 0.
 *     - `refine` rounds of a 65-way split: t_l = za + ((float)(l + 1) / 65.0f) * (zb - za), l = 0..63, g_l = g(t_l); the first adjacent pair of
 *       a, t_0 .. t_63, b that is (outside, inside) becomes the bracket (one always exists).
 *     - w = fminf(fmaxf((iso - ga) / (gb - ga), 0), 1), z* = za + w * (zb - za); depth = z*, in the units of z.
 *     - at p* = o + d z*: color = channels 1..3 of the interpolation.  The gradient is a central difference in grid coordinates with clamped
 *       steps: with u the clamped grid coordinate of p*, per axis a: u+ = fminf(u_a + 1, n_a - 1), u- = fmaxf(u_a - 1, 0),
 *       G_a = (f(u with u_a = u+) - f(u with u_a = u-)) / ((u+ - u-) * spacing_a) -- exact for an affine field, the border included.
 *       m = max |G_a|; m == 0 or not finite: the normal and n . v are 0.  Otherwise G /= m (so 1e30 voxels cannot overflow the squares),
 *       n = G / sqrtf(Gx^2 + Gy^2 + Gz^2), which points towards growing f (outward), and n . v = fmaxf(0, -((n . d) / |d|)).
 * One wave per ray, the samples over the lanes in rounds of 64 (the last value of a round carried into the next), "outside, then inside" a
 * 64-bit ballot whose lowest set bit is the crossing; the march stops at the first round that finds one.  March and refinement read channel 0
 * only.  All pointers but origin and spacing are DEVICE pointers.  All work goes to `stream`; no allocation, no host synchronisation, no
 * atomics, no device-side state; every output element is written on every call: the same bits every call.  Arguments are checked before any
 * launch.  One launch.                                                                                                                     */
int vanerf_volume_surface(const float* voxels, const float origin[3], const float spacing[3], int nx, int ny, int nz, float iso, int refine,
                          const float* rays_d, const float* cam_pos, const float* z, const uint8_t* hit, int R, int rays_per_view, int row_rays, int S,
                          float* depth, float* normal, float* color, uint8_t* found, void* stream);

/* The baked volume rendered in ANOTHER POSE of the same mesh.  The volume is a field in the source pose's space; the
 * mesh has the same faces in every pose; so a sample of a ray through the posed hand is carried back into source space by the affine map of
 * its closest face and looked up there.  A preview under the usual surface-aligned deformation model: it does not claim what the networks would
 * render from a photograph of the new pose.
 *
 *     vanerf_pose_transforms: verts_src[nv][3], verts_pose[nv][3], faces[nf][3] -> T[nf][12], one record per face: A (3 x 3, row-major) then
 *         t, the map q = A p + t from POSED space to SOURCE space.  For face (i0, i1, i2) and a mesh X: a = x1 - x0, b = x2 - x0, c = a x b,
 *         n = c / |c|, M_X = [a b n] as columns; the rows of M_X^-1 are (b x n) / det, (n x a) / det and n with det = a . (b x n).
 *         A = M_src M_pose^-1, t = x0_src - A x0_pose.  n is a UNIT vector: distance along the face normal is preserved, so skin thickness does
 *         not scale with the triangle's area.  Computed in fp64 from the fp32 vertices (every product and sum rounded separately, sums from the
 *         left) and rounded once to fp32.  A face whose |c|^2 is not above 1e-30 in either mesh, or any of whose 12 fp32 values is not finite,
 *         gets A = I, t = centroid_src - centroid_pose (centroid = ((x0 + x1) + x2) / 3 in fp64); a face with a vertex index outside
 *         [0, nv) gets A = I, t = 0.  nv, nf >= 1; T 16-byte aligned.  One thread per face, one launch.
 *     vanerf_volume_render_posed: vanerf_volume_render's grid, rays, sigmoid_beta, layouts and outputs, plus T[nf][12] (16-byte aligned), and
 *         per sample face[R][S] and sdf[R][S]: what vanerf_mesh_query_accel returns for the POSED mesh at the points of vanerf_sample_points on
 *         the same rays.  The kernel makes no discrete geometric decision of its own.  Per ray:
 *         - hit == 0: colour, depth and alpha are 0 and nothing else happens;
 *         - sample i is EMPTY iff face < 0, face >= nf, sdf is not finite or sdf > reach (reach: any float but NaN; +inf disables the test,
 *           -inf empties every sample).  An empty sample has c = 0: it contributes nothing and leaves the transmittance as it is;
 *         - otherwise p = o + d z_i per axis (vanerf_sample_points' expression) is carried to q = A p + t with its face's record, in fp32:
 *           qx = ((A00 px + A01 py) + A02 pz) + tx and likewise for y and z, every product and sum rounded separately; (f, r, g, b) is
 *           vanerf_volume_render's trilinear interpolation at q, with its clamp to the grid (border padding: given (face, sdf) the outputs
 *           are a continuous function of the float inputs; `reach` bounds how far a border voxel can smear) and its (1 - w) a + w b blends;
 *         - the composite is vanerf_volume_render's unchanged, dist = 1e10f for the ray's last sample whether or not that sample is empty.
 *         One wave per ray, the samples over the lanes in rounds of 64, the waves of a block on a 2 x 2 pixel tile of one view; a round all of
 *         whose samples are empty issues no gather (the same bits either way).  Any S >= 1; nf >= 1; V <= 65535; R == 0 is a no-op.  One launch.
 * All pointers but origin and spacing are DEVICE pointers.  All work goes to `stream`; no allocation, no host synchronisation, no atomics, no
 * device-side state; every output element is written on every call: the same bits every call.  Arguments are checked before any launch.  */
int vanerf_pose_transforms(const float* verts_src, const float* verts_pose, int nv, const int32_t* faces, int nf, float* T, void* stream);
int vanerf_volume_render_posed(const float* voxels, const float origin[3], const float spacing[3], int nx, int ny, int nz, const VanerfWeights* w,
                               float beta, const float* rays_d, const float* cam_pos, const float* z, const uint8_t* hit, int R, int rays_per_view,
                               int row_rays, int S, const float* T, int nf, const int32_t* face, const float* sdf, float reach, float* color,
                               float* depth, float* alpha, void* stream);

/* The surface of the baked volume as a camera sees it in ANOTHER POSE of the same mesh: vanerf_volume_surface's depth,
 * normal and colour maps along rays through the POSED hand.  The grid, rays, layouts, iso and refine (0 .. 4) are vanerf_volume_surface's;
 * T[nf][12], face[R][S], sdf[R][S] and reach are vanerf_volume_render_posed's; voxels, T and normal 16-byte aligned; any S >= 1; nf >= 1;
 * V <= 65535; R == 0 is a no-op.  -> depth[R], normal[R][4] = (nx, ny, nz, n . v), color[R][3], found[R] (0, 1, 2 or 3).  Per ray, all in fp32,
 * every product and sum its own operation:
 *     - hit == 0: found = 0 and every output is +0.
 *     - sample i is EMPTY by vanerf_volume_render_posed's rule, unchanged: face < 0, face >= nf, sdf not finite or sdf > reach.  For a face F,
 *       q_F(zz) = A_F p + t_F with p = o + d zz per axis, qx = ((A00 px + A01 py) + A02 pz) + tx and likewise for y and z, and g_F(zz) is
 *       channel 0 of vanerf_volume_render's trilinear interpolation at q_F(zz).  Sample i has g_i = g_face_i(z_i).  It is INSIDE iff it is not
 *       empty and g_i < iso: an empty sample is outside, and g == iso is outside.
 *     - sample 0 inside: found = 2, z* = z_0, F = face_0.  With S == 1 this is the only way to be found.
 *     - otherwise the smallest k with sample k not inside and sample k + 1 inside.  None: found = 0 and every output is +0.
 *       F = face_k+1: the map of the INSIDE end carries the whole bracket, because the refinement points have no mesh query of their own.
 *       za = z_k, zb = z_k+1, gb = g_k+1, and ga = g_F(z_k), re-evaluated under F whatever sample k was (empty, or carried by another face).
 *     - ga < iso: found = 3 and z* = za.  Under F's map the surface lies at or in front of sample k; the depth is held at the bracket's near
 *       end and nothing is refined.
 *     - otherwise found = 1: `refine` rounds of vanerf_volume_surface's 65-way split with g_F (one (outside, inside) pair always exists), then
 *       its linear step, w = fminf(fmaxf((iso - ga) / (gb - ga), 0), 1), z* = za + w * (zb - za).
 *     - at q* = q_F(z*): color = channels 1..3 of the interpolation, G = vanerf_volume_surface's clamped central difference of channel 0 in
 *       SOURCE space.  The normal in POSED space is the gradient of f(A p + t) with respect to p, N = A^T G:
 *       N_j = (A_0j G_0 + A_1j G_1) + A_2j G_2.  Then vanerf_volume_surface's normalisation of N (m = max |N_j|; m == 0 or not finite: the
 *       normal and n . v are 0; scaled by 1 / m first) and n . v = fmaxf(0, -((n . d) / |d|)) with the POSED ray's d.  depth = z*.
 * One wave per ray, the samples over the lanes in rounds of 64 ("was the last sample inside" carried into the next), coalesced loads of face
 * and sdf and three 16-byte loads of the record per live lane; a round all of whose samples are empty issues no gather (the same bits either
 * way); "not inside there, inside here" is a 64-bit ballot, the march stops at the first round with a crossing, and F comes by shuffle from
 * the crossing lane: from there on the record is wave-uniform.  All pointers but origin and spacing are DEVICE pointers.  All work goes to
 * `stream`; no allocation, no host synchronisation, no atomics, no device-side state; every output element is written on every call: the same
 * bits every call.  Arguments are checked before any launch.  One launch.                                                                  */
int vanerf_volume_surface_posed(const float* voxels, const float origin[3], const float spacing[3], int nx, int ny, int nz, float iso, int refine,
                                const float* rays_d, const float* cam_pos, const float* z, const uint8_t* hit, int R, int rays_per_view, int row_rays,
                                int S, const float* T, int nf, const int32_t* face, const float* sdf, float reach, float* depth, float* normal,
                                float* color, uint8_t* found, void* stream);

/* Linear blend skinning of a MANO-shaped model for a batch of P poses: pose, shape and translation parameters -> the
 * vertices and joints of every pose, on the device, with no host read.  What follows is the definition (it is what smplx 0.1.x computes with
 * lbs and pose2rot = True, restated so that nothing here points anywhere else).
 *
 * The MODEL has nv vertices, nj joints (1 .. 32) and nb shape coefficients (1 .. 16), and carries, all fp32 and row-major:
 *     v_template[nv][3];  shapedirs[nv][3][nb];  posedirs[(nj-1)*9][nv*3]: row (j-1)*9 + 3r + c belongs to joint j >= 1 and entry (r, c) of its
 *     rotation, column 3v + k to vertex v and coordinate k;  J_regressor[nj][nv];  weights[nv][nj];  hands_mean[(nj-1)*3];  and parents[nj]
 *     (int32) with parents[0] = -1 and 0 <= parents[j] < j.  With nj = 1 posedirs and hands_mean are empty and may be null.
 * For one pose row pose[nj*3] (axis-angle per joint, the root first), betas[nb] and trans[3]:
 *     1. full = pose; unless flat_hand_mean is set, full[3:] += hands_mean.
 *     2. v_shaped = v_template + shapedirs . betas;  J = J_regressor . v_shaped  (= J_regressor . v_template + (J_regressor . shapedirs) . betas).
 *     3. per joint j, with r = full[3j .. 3j+2]: angle = sqrt((r0 + 1e-8)^2 + (r1 + 1e-8)^2 + (r2 + 1e-8)^2) -- the constant is added to every
 *        component and enters the norm only -- d = r / angle, K = [[0, -d2, d1], [d2, 0, -d0], [-d1, d0, 0]] and
 *        R_j = I + sin(angle) K + (1 - cos(angle)) K K.  r = 0 gives R_j = I exactly.
 *     4. v_posed = v_shaped + posedirs^T . f, the pose feature f[(j-1)*9 + 3r + c] = (R_j - I)[r][c] for j = 1 .. nj-1.
 *     5. the chain: L_j = [R_j | J_j - J_parents[j]] (3 x 4; J_0 itself for the root), G_0 = L_0 and G_j = G_parents[j] L_j as rigid maps
 *        (G^R = Gp^R L^R, G^t = Gp^R L^t + Gp^t).  A_j = [G_j^R | G_j^t - G_j^R J_j].
 *     6. vertex v = (sum_j weights[v][j] A_j) . (v_posed_v, 1) + trans;  joint j = G_j^t + trans.
 *     7. the seal (n_ring > 0): ONE more vertex, index nv, is appended: the mean of the vertices ring[0 .. n_ring-1].  Its arithmetic is fixed:
 *        in fp32, s = x[ring[0]], then s = s + x[ring[u]] for u = 1 .. n_ring-1 over the vertices as WRITTEN by this call, times
 *        (1.0f / (float)n_ring) -- so the appended vertex equals that expression of the call's own output bit for bit.
 * Where the arithmetic happens: steps 1, 3, 5, J of step 2 and the joints of step 6 in fp64 (sin, cos and sqrt of the device's fp64 library),
 * sums from the left, each rounded ONCE to fp32: A, f and the joints.  Steps 2 (v_shaped), 4 and the vertices of step 6 in fp32, every
 * product and sum its own IEEE operation, in this order: s = 0, s = s + shapedirs[v][k][b] * betas[b] for b = 0 .. nb-1, x = v_template + s;
 * o = 0, o = o + posedirs[row][3v+k] * f[row] for row = 0 .. (nj-1)*9 - 1, x = x + o; T = 0, T = T + weights[v][j] * A_j for j = 0 .. nj-1 (no
 * term is skipped: a NaN or an infinity in a pose's parameters reaches every vertex of that pose, and no other pose);
 * out_k = ((T_k0 x_0 + T_k1 x_1) + T_k2 x_2) + T_k3, then out_k + trans_k.  A pose's bits depend neither on P nor on its row in the batch.
 *
 *     vanerf_mano_packed_bytes (nv, nj, nb) -> the size of a model's packed tables;  vanerf_mano_workspace_bytes (nj, P) -> the workspace of a
 *         call with P poses;  vanerf_mano_poses_per_lane () -> how many poses a lane of the vertex kernel carries (P just below, at and above it
 *         are the batch sizes at which a block's last poses are, or are not, past the batch).  Host only; bad sizes give a negative error code.
 *     vanerf_mano_pack: the model's arrays (DEVICE pointers; parents a HOST pointer, checked here) -> packed (DEVICE, 16-byte aligned, at least
 *         vanerf_mano_packed_bytes): the tables transposed to [row][k][v], J_regressor . v_template and J_regressor . shapedirs in fp64 (sums
 *         over the vertices from vertex 0), hands_mean as doubles and the parents.  Once per model; two launches.  The known sign error of the
 *         left hand's shapedirs in the files smplx reads is the caller's data preparation: nothing is flipped here.
 *     vanerf_mano_skin: packed with the SAME nv, nj, nb, and pose, betas, trans as P rows `*_stride` floats apart (DEVICE) -> verts: P rows
 *         verts_stride floats apart, each (nv + (n_ring > 0)) x 3 floats, and joints: P rows joints_stride floats apart, each nj x 3 floats.
 *         The strides let the right and the left hand read from, and write into, the halves of one tensor.  Every stride is at least its
 *         row's length; rows must not overlap.  ring: a HOST pointer to n_ring ids in [0, nv), 0 <= n_ring <= 64; n_ring = 0: no seal (ring
 *         may be null).  workspace: DEVICE, at least vanerf_mano_workspace_bytes, contents undefined before and after.  P = 0 is valid and a
 *         no-op.  Launches: one wave per pose for the joints, one lane per vertex carrying several poses for the vertices, one thread per
 *         pose and coordinate for the seal.
 * All work goes to `stream`; no allocation, no host synchronisation, no atomics, no device-side state; every output element is written on every
 * call: the same bits every call.  Arguments are checked before any launch.                                                               */
int64_t vanerf_mano_packed_bytes(int nv, int nj, int nb);
int64_t vanerf_mano_workspace_bytes(int nj, int P);
int vanerf_mano_poses_per_lane(void);
int vanerf_mano_pack(const float* v_template, const float* shapedirs, const float* posedirs, const float* J_regressor, const float* weights,
                     const int32_t* parents, const float* hands_mean, int nv, int nj, int nb, void* packed, int64_t packed_bytes, void* stream);
int vanerf_mano_skin(const void* packed, int nv, int nj, int nb, const float* pose, int64_t pose_stride, const float* betas, int64_t betas_stride,
                     const float* trans, int64_t trans_stride, int P, int flat_hand_mean, const int32_t* ring, int n_ring, void* workspace,
                     int64_t workspace_bytes, float* verts, int64_t verts_stride, float* joints, int64_t joints_stride, void* stream);

/* The vector-Jacobian product of vanerf_mano_skin: the gradients of a scalar with respect to the vertices and joints of
 * P poses -> its gradients with respect to pose, betas and trans, on the device, with no host read.  The function differentiated is the
 * definition above exactly as written, steps 1-7: the constant 1e-8 sits in the angle (so the gradient at r = 0 is finite: sin(angle) / angle
 * is), hands_mean is an additive constant, and the seal passes (1.0f / (float)n_ring) of the appended vertex's gradient to ring[u] for EVERY
 * u, so an id that the ring repeats receives it as often as it occurs.  The roundings of the forward are not differentiated.
 *
 * Stateless: R, J, the chain, A, the pose feature, v_posed and T are recomputed from pose and betas (the forward's arithmetic and bits); nothing
 * is taken from a forward call, and trans is not an input.  packed, nv, nj, nb, pose, betas, P, flat_hand_mean, ring and n_ring are the
 * forward's.  grad_verts: P rows grad_verts_stride floats apart, each (nv + (n_ring > 0)) x 3 floats; grad_joints: P rows of nj x 3 floats.
 * Either may be null, which is read as zeros; both null is an error.  grad_pose (P rows of nj x 3), grad_betas (P rows of nb) and grad_trans
 * (P rows of 3), each with its own stride: any may be null, which means not wanted, and every element of the others is written.  The strides
 * let one hand address its half of a (P, 2, .) tensor; every stride is at least its row's length.  workspace: DEVICE, 8-byte aligned, at least
 * vanerf_mano_skin_backward_workspace_bytes (nv, nj, nb, P), contents undefined before and after (not read when grad_verts is null).  P = 0
 * is valid and a no-op.
 *
 * Where the arithmetic happens.  Vertex side, fp32, every product and sum its own IEEE operation: x = v_posed and T as the forward computes
 * them; g = the vertex's gradient, then g = g + (grad of the appended vertex) * (1.0f / n_ring) once per occurrence in the ring's order;
 * g_x[c] = (T_0c g_0 + T_1c g_1) + T_2c g_2.  The sums over the vertices -- dA_j[r][c] = sum_v (w_vj g_r) (x_c | 1), df[row] = sum_v sum_k
 * posedirs[row][3v+k] g_x[k], the direct part of grad_betas = sum_v sum_k shapedirs[v][k][b] g_x[k], and sum_v g -- take fp32 products and
 * add them in fp64: per chunk of 256 vertices, lane l of a wave adds its vertices l, l + 64, l + 128, l + 192 (k innermost), a butterfly adds
 * the 64 lanes, and the chunks' sums are added in chunk order.  Joint side, fp64: dG_j^t = dA_j^t + grad_joint_j, dG_j^R = dA_j^R - dA_j^t
 * J_j^T, dJ_j = -G_j^R^T dA_j^t; for j = nj-1 .. 1 with p = parents[j]: dR_j = G_p^R^T dG_j^R, dG_p^R += dG_j^R R_j^T + dG_j^t (J_j - J_p)^T,
 * dl = G_p^R^T dG_j^t, dJ_j += dl, dJ_p -= dl, dG_p^t += dG_j^t; the root: dR_0 = dG_0^R, dJ_0 += dG_0^t; dR_j += df_j for j >= 1; the
 * Rodrigues backward of step 3 gives grad_pose; grad_betas = direct part + (J_regressor . shapedirs)^T dJ; grad_trans = sum_v g + sum_j
 * grad_joint_j.  Each output is rounded once to fp32.  A pose's gradient bits depend neither on P nor on its row in the batch; a NaN in one
 * pose's gradients stays in that pose.
 * Three launches (one when grad_verts is null).  All work goes to `stream`; no allocation, no host synchronisation, no atomics, no device-side
 * state: the same bits every call.  Arguments are checked before any launch.                                                              */
int64_t vanerf_mano_skin_backward_workspace_bytes(int nv, int nj, int nb, int P);
int vanerf_mano_skin_backward(const void* packed, int nv, int nj, int nb, const float* pose, int64_t pose_stride, const float* betas,
                              int64_t betas_stride, int P, int flat_hand_mean, const int32_t* ring, int n_ring, const float* grad_verts,
                              int64_t grad_verts_stride, const float* grad_joints, int64_t grad_joints_stride, void* workspace,
                              int64_t workspace_bytes, float* grad_pose, int64_t grad_pose_stride, float* grad_betas, int64_t grad_betas_stride,
                              float* grad_trans, int64_t grad_trans_stride, void* stream);

/* The normal equations of fitting vanerf_mano_skin to a mesh: what one Gauss-Newton / Levenberg-Marquardt iteration
 * needs, on the device, with no host read.  The unknowns of a pose are ordered x = (pose[3 nj], betas[nb], trans[3]), n = 3 nj + nb + 3 (at most
 * 115).  The residuals are r = (v - v*, j - j*): the (nv + (n_ring > 0)) vertices of the definition above, steps 1-7, against target_verts, then
 * the nj joints against target_joints; the sealed vertex is a residual like any other.  The weights are W = (w_v / nv_out, 1 / nj) with
 * nv_out = nv + (n_ring > 0) and w_v = vert_weight[v] (null: ones), each repeated for its three coordinates.  With J = dr/dx, per pose:
 *     H = J^T W J   (n x n, fp32, the full symmetric matrix: both triangles are written and equal bit for bit),
 *     g = J^T W r   (n),        loss = r^T W r   (a scalar).
 * So mean_v w_v |v - v*|^2 + mean_j |j - j*|^2 = loss, and its gradient is 2 g.  J is the derivative of the definition exactly as
 * vanerf_mano_skin_backward differentiates it: the 1e-8 sits in the angle, hands_mean is additive, the seal's rows are (1.0f / (float)n_ring)
 * times the sum of its ring's rows, once per occurrence, and the forward's roundings are not differentiated.
 *
 * packed, nv, nj, nb, pose, betas, trans, P, flat_hand_mean, ring and n_ring are the forward's.  target_verts: P rows target_verts_stride
 * floats apart, each nv_out x 3; target_joints: P rows of nj x 3.  Either may be null, which takes its residuals out; both null is an error.
 * vert_weight: P rows of nv_out floats, vert_weight_stride apart; a stride of 0 means one row shared by all poses; null means ones (and it
 * must be null when target_verts is).  Weights are expected to be >= 0.  H: P matrices H_stride floats apart (at least n * n), row-major;
 * g: P rows g_stride apart; loss: P scalars loss_stride apart.  Any of H, g, loss may be null, which means not written; every element of the
 * others is written.  workspace: DEVICE, 16-byte aligned, at least vanerf_mano_skin_normal_workspace_bytes (nv, nj, nb, P), contents
 * undefined before and after.  P = 0 is valid and a no-op.  Stateless: nothing is taken from a forward call.
 *
 * Where the arithmetic happens.  Joint side, fp64, one wave per pose: steps 1, 3, 5 and J of step 2 as the forward computes them (A and the
 * pose feature have the forward's bits), the derivative dR_a/dr_x of step 3, D_ax = G_parents[a]^R dR_a/dr_x G_a^R^-1 (the inverse by
 * cofactors: with the 1e-8 in the angle R is orthogonal only to 1e-8 |r|; the root: dR_0/dr_x G_0^R^-1), G_a^t, and down the chain
 * dG_j^t/dbeta_b = G_p^R ((JS)_j - (JS)_p)_b + dG_p^t/dbeta_b with JS = J_regressor . shapedirs, dA_j^t/dbeta_b
 * = dG_j^t/dbeta_b - G_j^R (JS)_jb; each rounded ONCE to fp32.  A pose parameter (a, x) moves A_j for j = a and every joint below a, by
 * dA_j = D_ax [A_j^R | A_j^t - G_a^t], and no other; so the tables do not grow with the depth of the tree.
 * Vertex side, fp32, every product and sum its own IEEE operation unless said otherwise: x = v_posed, T and the vertex as the forward computes
 * them (the residual is the forward's vertex minus its target).  Column (a, x) of a vertex's 3 x n block of J: S = sum over j = a .. nj-1
 * that are a or below it, in that order, of w_vj (A_j (x, 1)), Ws = the sum of those w_vj, u = S - Ws G_a^t, column = D_ax u + T^R (sum over
 * e = 0 .. 8 of posedirs[(a-1)*9 + e][3v + .] dR_a/dr_x[e]) (the second term for a >= 1).  Column of beta_b: T^R shapedirs[v][.][b] + sum over
 * j from 0 of w_vj dA_j^t/dbeta_b.  The columns of trans: the identity.  The sealed vertex: the rows of ring[0 .. n_ring-1] recomputed, added
 * in the ring's order from the left and multiplied by (1.0f / (float)n_ring), on every column and on the position (the forward's sum).
 * The sums over the residual rows: per chunk of 64 vertices (the sealed vertex is a chunk of its own, the last), over the chunk's 192 rows in
 * the order coordinate-major, vertex-minor, acc = fmaf(a, w * b, acc) in fp32 -- an fp32 product w * b, then a FUSED multiply-add: the chain
 * the exact-fp32 matrix instruction v_mfma_f32_32x32x2_f32 computes per element, two rows per instruction -- for the lower triangle of
 * (J | r)^T W (J | r) -- but r^T W r itself, one entry, as (double)(w * r) * (double)r added in fp64, a lane's three rows from coordinate 0,
 * then a butterfly over the 64 lanes, rounded to fp32 per chunk --; the chunks' sums are added in chunk order in fp64; the joints' rows
 * (dG_j^t/dx = D_ax (G_j^t - G_a^t)
 * for a above j, dG_j^t/dbeta_b, the identity; r_j = the forward's fp32 joint minus its target) are multiplied and added in fp64, row by row,
 * and divided by nj; one rounding to fp32.  The upper triangle of H is a copy of the lower.  A pose's bits depend neither on P nor on its
 * row in the batch; a NaN in one pose's inputs stays in that pose.
 * Three launches (two when target_verts is null).  All work goes to `stream`; no allocation, no host synchronisation, no atomics, no
 * device-side state: the same bits every call.  Arguments are checked before any launch.
 *
 * vanerf_mano_lm_solve: delta = -M^-1 g for P symmetric positive definite systems of 1 <= n <= 128 unknowns.  M: P matrices M_stride floats
 * apart (at least n * n), row-major, of which the LOWER triangle is read; g, delta: P rows with their strides (at least n); ok: P int32.  One
 * wave per system, the matrix in LDS in fp64: Cholesky column by column (s = M_ij, s = s - L_ik L_jk for k = 0 .. j-1), the two triangular
 * solves, one rounding to fp32.  A pivot that is not positive or not finite, or a result that is not finite, gives that system ok = 0 and
 * delta = 0; the others are untouched; otherwise ok = 1.  No host read; P = 0 is a no-op; one launch on `stream`.                          */
int64_t vanerf_mano_skin_normal_workspace_bytes(int nv, int nj, int nb, int P);
int vanerf_mano_skin_normal(const void* packed, int nv, int nj, int nb, const float* pose, int64_t pose_stride, const float* betas,
                            int64_t betas_stride, const float* trans, int64_t trans_stride, int P, int flat_hand_mean, const int32_t* ring, int n_ring,
                            const float* target_verts, int64_t target_verts_stride, const float* vert_weight, int64_t vert_weight_stride,
                            const float* target_joints, int64_t target_joints_stride, void* workspace, int64_t workspace_bytes, float* H,
                            int64_t H_stride, float* g, int64_t g_stride, float* loss, int64_t loss_stride, void* stream);
int vanerf_mano_lm_solve(const float* M, int64_t M_stride, const float* g, int64_t g_stride, int n, int P, float* delta, int64_t delta_stride,
                         int32_t* ok, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* VANERF_HIP_H */
