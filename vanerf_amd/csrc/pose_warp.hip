// pose_warp.hip -- the baked volume rendered in another pose of the same mesh (the comments of vanerf_pose_transforms /
// vanerf_volume_render_posed in the header).  The volume is a field in the SOURCE pose's space and the mesh has the same faces in every pose,
// so a sample of a ray through the POSED hand is carried back into source space by the affine map of its closest face and looked up there:
// no network per view, and the only per-sample geometry work is the mesh query the library already has, whose outputs (face, sdf) this file
// takes as inputs.  A preview under the usual surface-aligned deformation model, not what the networks would render from a photograph of the
// new pose.  The restatement the tests hold these kernels to is the numpy code of tests/test_posed_volume_cpu.py.
//
// The march restates volume_render_kernel's pattern (volume_render.hip): one wave per ray, lanes over samples in rounds of 64, the
// transmittance an exclusive prefix product with a fixed shuffle pattern, the sums a fixed xor butterfly in fp64.  New per lane and round:
// the coalesced loads of face and sdf, three 16-byte loads of the face's record and nine multiplies.  The table of records (nf x 48 bytes,
// 149 KB for the two-hand mesh) stays in L2 and is shared by every wave; it is NOT staged in LDS, which it would fill, taking the occupancy
// that hides the gathers.  No atomics, no device-side state, no LDS.  Built with -ffp-contract=off: every product and sum is its own IEEE
// operation.
#include "common.h"

#include <cfloat>
#include <cmath>
#include <cstdint>

using namespace vanerf;

namespace {

constexpr int PT_BLOCK = 256;
constexpr int PT_FLOATS = 12;        // a face's record: A row-major, then t
constexpr double PT_MIN_AREA2 = 1e-30; // |a x b|^2 at or below this: the face has no frame

struct Frame64 {
    double x0[3], a[3], b[3], n[3], c2, cen[3];
};

__device__ __forceinline__ void cross64(const double* u, const double* v, double* o)
{
    o[0] = u[1] * v[2] - u[2] * v[1];
    o[1] = u[2] * v[0] - u[0] * v[2];
    o[2] = u[0] * v[1] - u[1] * v[0];
}

__device__ __forceinline__ double dot64(const double* u, const double* v) { return (u[0] * v[0] + u[1] * v[1]) + u[2] * v[2]; }

__device__ __forceinline__ Frame64 frame_of(const float* __restrict__ X, int i0, int i1, int i2)
{
    Frame64 F;
    double c[3];
    for (int k = 0; k < 3; ++k) {
        const double p0 = (double)X[3 * (size_t)i0 + k], p1 = (double)X[3 * (size_t)i1 + k], p2 = (double)X[3 * (size_t)i2 + k];
        F.x0[k] = p0;
        F.a[k] = p1 - p0;
        F.b[k] = p2 - p0;
        F.cen[k] = ((p0 + p1) + p2) / 3.0;
    }
    cross64(F.a, F.b, c);
    F.c2 = dot64(c, c);
    const double len = sqrt(F.c2);
    for (int k = 0; k < 3; ++k) F.n[k] = c[k] / len;
    return F;
}

// One thread per face, everything in fp64 from the fp32 vertices, rounded once.  T[f] = (A row-major, t) with A = M_src M_pose^-1,
// t = x0_src - A x0_pose: posed space -> source space.  M = [a b n] with n the UNIT normal, so the rows of M^-1 are (b x n) / det,
// (n x a) / det and n with det = a . (b x n).
__global__ __launch_bounds__(PT_BLOCK) void pose_transforms_kernel(const float* __restrict__ verts_src, const float* __restrict__ verts_pose, int nv,
                                                                   const int32_t* __restrict__ faces, int nf, float4* __restrict__ T)
{
    const int f = blockIdx.x * PT_BLOCK + threadIdx.x;
    if (f >= nf) return;
    const int i0 = faces[3 * (size_t)f], i1 = faces[3 * (size_t)f + 1], i2 = faces[3 * (size_t)f + 2];
    float o[PT_FLOATS] = {1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f}; // a face that names no vertex: the identity
    if (i0 >= 0 && i0 < nv && i1 >= 0 && i1 < nv && i2 >= 0 && i2 < nv) {
        const Frame64 Fs = frame_of(verts_src, i0, i1, i2), Fp = frame_of(verts_pose, i0, i1, i2);
        double bn[3], na[3], r[3][3];
        cross64(Fp.b, Fp.n, bn);
        cross64(Fp.n, Fp.a, na);
        const double det = dot64(Fp.a, bn);
        for (int j = 0; j < 3; ++j) { r[0][j] = bn[j] / det; r[1][j] = na[j] / det; r[2][j] = Fp.n[j]; }
        float m[PT_FLOATS];
        bool ok = Fs.c2 > PT_MIN_AREA2 && Fp.c2 > PT_MIN_AREA2; // (NaN compares false)
        for (int i = 0; i < 3; ++i) {
            double A[3];
            for (int j = 0; j < 3; ++j) A[j] = (Fs.a[i] * r[0][j] + Fs.b[i] * r[1][j]) + Fs.n[i] * r[2][j];
            const double t = Fs.x0[i] - ((A[0] * Fp.x0[0] + A[1] * Fp.x0[1]) + A[2] * Fp.x0[2]);
            for (int j = 0; j < 3; ++j) m[3 * i + j] = (float)A[j];
            m[9 + i] = (float)t;
        }
        for (int k = 0; k < PT_FLOATS; ++k) ok = ok && fabsf(m[k]) <= FLT_MAX;
        for (int k = 0; k < PT_FLOATS; ++k) o[k] = ok ? m[k] : o[k];
        if (!ok)
            for (int k = 0; k < 3; ++k) o[9 + k] = (float)(Fs.cen[k] - Fp.cen[k]); // A = I, t = centroid_src - centroid_pose
    }
    T[3 * (size_t)f] = make_float4(o[0], o[1], o[2], o[3]);
    T[3 * (size_t)f + 1] = make_float4(o[4], o[5], o[6], o[7]);
    T[3 * (size_t)f + 2] = make_float4(o[8], o[9], o[10], o[11]);
}

struct VolGrid {
    float o[3], s[3];
    int nx, ny, nz;
};

constexpr int PW_TX = 2, PW_TY = 2; // the pixel tile of a block: neighbouring pixels meet the same faces and cells, so their gathers share cache lines
constexpr int PW_WAVES = PW_TX * PW_TY;
#ifdef VANERF_POSED_NO_SKIP
constexpr bool PW_SKIP = false;
#else
constexpr bool PW_SKIP = true;
#endif

// volume_render.hip's grid coordinate: clamped onto the grid (border padding; fmaxf(NaN, 0) is 0, so no address leaves the grid)
__device__ __forceinline__ void cell_of(float p, float origin, float spacing, int n, int& i0, float& w)
{
    float u = (p - origin) / spacing;
    u = fminf(fmaxf(u, 0.0f), (float)(n - 1));
    i0 = min((int)floorf(u), n - 2);
    w = u - (float)i0;
}

__device__ __forceinline__ float4 blend(float w, const float4& a, const float4& b)
{
    const float k = 1.0f - w;
    float4 o;
    o.x = k * a.x + w * b.x; o.y = k * a.y + w * b.y; o.z = k * a.z + w * b.z; o.w = k * a.w + w * b.w;
    return o;
}

// One wave per ray, lane l of round k holds sample 64 k + l; block (bx, by) of view blockIdx.y takes the PW_TX x PW_TY pixels at
// (PW_TX bx, PW_TY by) of the view's row_rays-wide ray grid.  A sample is EMPTY (c = 0) iff face < 0, face >= nf, sdf is not finite or
// sdf > reach; the others are carried to q = A p + t by their face's record and interpolated there.  SKIP: a round all of whose samples are
// empty -- most of a ray is farther than `reach` from the hand -- issues no gather; the bits are the same either way, an empty sample has
// c = 0 with or without the branch (a build with -DVANERF_POSED_NO_SKIP takes it out, to show that and to time it: tools/perf_posed.py).
__global__ __launch_bounds__(64 * PW_WAVES) void volume_render_posed_kernel(const float4* __restrict__ voxels, const VolGrid G, float beta,
                                                                            const float* __restrict__ beta_dev, const float* __restrict__ rays_d,
                                                                            const float* __restrict__ cam_pos, const float* __restrict__ z,
                                                                            const uint8_t* __restrict__ hit, int rays_per_view, int row_rays, int S,
                                                                            const float4* __restrict__ T, int nf, const int32_t* __restrict__ face,
                                                                            const float* __restrict__ sdf, float reach, float* __restrict__ color,
                                                                            float* __restrict__ depth, float* __restrict__ alpha)
{
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int tiles_x = (row_rays + PW_TX - 1) / PW_TX;
    const int px = (int)(blockIdx.x % tiles_x) * PW_TX + (wave % PW_TX);
    const int py = (int)(blockIdx.x / tiles_x) * PW_TY + (wave / PW_TX);
    if (px >= row_rays || py >= rays_per_view / row_rays) return; // whole wave
    const int v = blockIdx.y;
    const size_t r = (size_t)v * (size_t)rays_per_view + (size_t)py * (size_t)row_rays + (size_t)px;
    if (!hit[r]) { // whole wave: the ray misses the box
        if (lane == 0) { color[3 * r] = 0.0f; color[3 * r + 1] = 0.0f; color[3 * r + 2] = 0.0f; depth[r] = 0.0f; alpha[r] = 0.0f; }
        return;
    }
    if (beta_dev) beta = *beta_dev; // a weight handle's device copy of sigmoid_beta, already clamped
    const float ox = cam_pos[4 * v], oy = cam_pos[4 * v + 1], oz = cam_pos[4 * v + 2];
    const float dx = rays_d[3 * r], dy = rays_d[3 * r + 1], dz = rays_d[3 * r + 2];
    const float* zr = z + r * (size_t)S;
    const int32_t* fr = face + r * (size_t)S;
    const float* sr = sdf + r * (size_t)S;
    const size_t row = (size_t)G.nx, slab = (size_t)G.nx * (size_t)G.ny;
    double cr = 0, cg = 0, cb = 0, ca = 0, cd = 0;
    float carry = 1.0f; // the transmittance in front of this round's first sample
    for (int i0 = 0; i0 < S; i0 += 64) { // (S is uniform: every lane runs every round)
        const int i = i0 + lane;
        float c = 0.0f, zi = 0.0f;
        float4 q = {0.0f, 0.0f, 0.0f, 0.0f};
        int fi = -1;
        float sd = 0.0f;
        if (i < S) { zi = zr[i]; fi = fr[i]; sd = sr[i]; }
        const bool live = fi >= 0 && fi < nf && fabsf(sd) <= FLT_MAX && sd <= reach; // (NaN compares false)
        if (!PW_SKIP || __ballot(live) != 0ull) { // wave-uniform
            if (live) {
                const float dist = i + 1 < S ? zr[i + 1] - zi : 1e10f;
                const float4* t = T + 3 * (size_t)fi;
                const float4 t0 = t[0], t1 = t[1], t2 = t[2]; // A00 A01 A02 A10 | A11 A12 A20 A21 | A22 tx ty tz
                const float ppx = ox + dx * zi, ppy = oy + dy * zi, ppz = oz + dz * zi; // p = o + d z per axis: sample_points_kernel's expression
                const float qx = ((t0.x * ppx + t0.y * ppy) + t0.z * ppz) + t2.y;
                const float qy = ((t0.w * ppx + t1.x * ppy) + t1.y * ppz) + t2.z;
                const float qz = ((t1.z * ppx + t1.w * ppy) + t2.x * ppz) + t2.w;
                int ix, iy, iz;
                float wx, wy, wz;
                cell_of(qx, G.o[0], G.s[0], G.nx, ix, wx);
                cell_of(qy, G.o[1], G.s[1], G.ny, iy, wy);
                cell_of(qz, G.o[2], G.s[2], G.nz, iz, wz);
                const float4* p = voxels + (((size_t)iz * (size_t)G.ny + (size_t)iy) * row + (size_t)ix);
                const float4 v000 = p[0], v100 = p[1], v010 = p[row], v110 = p[row + 1];
                const float4 v001 = p[slab], v101 = p[slab + 1], v011 = p[slab + row], v111 = p[slab + row + 1];
                q = blend(wz, blend(wy, blend(wx, v000, v100), blend(wx, v010, v110)), blend(wy, blend(wx, v001, v101), blend(wx, v011, v111)));
                const float a = q.x;
                const float sg = (1.0f / (1.0f + expf(-(-a / beta)))) / beta; // sigmoid(-a / beta) / beta, composite_kernel's expression
                c = 1.0f - expf(-sg * dist);
            }
        }
        // exclusive multiplicative scan of 1 - c over the lanes, behind the rounds before
        float incl = 1.0f - c;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float u = __shfl_up(incl, d);
            if (lane >= d) incl *= u;
        }
        float Tr = __shfl_up(incl, 1);
        if (lane == 0) Tr = 1.0f;
        Tr = carry * Tr;
        carry = carry * __shfl(incl, 63);
        const float w = c * Tr;
        if (i < S) {
            cr += (double)(q.y * w); cg += (double)(q.z * w); cb += (double)(q.w * w);
            ca += (double)w; cd += (double)(zi * w);
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        cr += __shfl_xor(cr, d); cg += __shfl_xor(cg, d); cb += __shfl_xor(cb, d);
        ca += __shfl_xor(ca, d); cd += __shfl_xor(cd, d);
    }
    if (lane == 0) {
        const float acc = (float)ca;
        color[3 * r] = (float)cr; color[3 * r + 1] = (float)cg; color[3 * r + 2] = (float)cb;
        alpha[r] = acc;
        depth[r] = (float)cd / (acc + 1e-8f);
    }
}

void check_grid(const char* who, const float* origin, const float* spacing, int nx, int ny, int nz)
{
    if (!origin || !spacing) throw_error("%s: null argument", who);
    if (nx < 2 || ny < 2 || nz < 2) throw_error("%s: a grid of (%d, %d, %d) points: every dimension must be at least 2", who, nx, ny, nz);
    if (7LL * nx * ny >= (1LL << 31) || 7LL * nx * ny * nz >= (1LL << 31))
        throw_error("%s: a grid of (%d, %d, %d) points is too large: 7 nx ny nz must stay below 2^31", who, nx, ny, nz);
    for (int a = 0; a < 3; ++a) {
        if (!std::isfinite(origin[a])) throw_error("%s: the grid origin must be finite", who);
        if (!(std::isfinite(spacing[a]) && spacing[a] > 0.0f)) throw_error("%s: the grid spacing must be finite and positive", who);
    }
}

} // namespace

extern "C" int vanerf_pose_transforms(const float* verts_src, const float* verts_pose, int nv, const int32_t* faces, int nf, float* T, void* stream)
{
    return guarded([&] {
        if (!verts_src || !verts_pose || !faces || !T) throw_error("vanerf_pose_transforms: null argument");
        if (nv < 1 || nf < 1) throw_error("vanerf_pose_transforms: nv=%d nf=%d (at least 1 each)", nv, nf);
        if ((uintptr_t)T & 15) throw_error("vanerf_pose_transforms: T must be 16-byte aligned");
        hipLaunchKernelGGL(pose_transforms_kernel, dim3((unsigned)((nf + PT_BLOCK - 1) / PT_BLOCK)), dim3(PT_BLOCK), 0, (hipStream_t)stream, verts_src,
                           verts_pose, nv, faces, nf, reinterpret_cast<float4*>(T));
        HIP_CHECK(hipGetLastError());
    });
}

extern "C" int vanerf_volume_render_posed(const float* voxels, const float origin[3], const float spacing[3], int nx, int ny, int nz,
                                          const VanerfWeights* w, float beta, const float* rays_d, const float* cam_pos, const float* z,
                                          const uint8_t* hit, int R, int rays_per_view, int row_rays, int S, const float* T, int nf,
                                          const int32_t* face, const float* sdf, float reach, float* color, float* depth, float* alpha, void* stream)
{
    return guarded([&] {
        const char* who = "vanerf_volume_render_posed";
        if (!voxels || !rays_d || !cam_pos || !z || !hit || !T || !face || !sdf || !color || !depth || !alpha) throw_error("%s: null argument", who);
        check_grid(who, origin, spacing, nx, ny, nz);
        if (((uintptr_t)voxels & 15) || ((uintptr_t)T & 15)) throw_error("%s: voxels and T must be 16-byte aligned", who);
        if (S < 1) throw_error("%s: S = %d samples per ray (at least 1)", who, S);
        if (nf < 1) throw_error("%s: nf = %d faces (at least 1)", who, nf);
        if (std::isnan(reach)) throw_error("%s: reach must not be NaN (+inf disables it)", who);
        if (w && !w->dev_beta) throw_error("%s: the weight handle carries no sigmoid_beta", who);
        if (!w && !(std::isfinite(beta) && beta > 0.0f)) throw_error("%s: beta must be finite and positive", who);
        if (R < 0 || rays_per_view < 1 || row_rays < 1) throw_error("%s: R=%d rays_per_view=%d row_rays=%d", who, R, rays_per_view, row_rays);
        if (R % rays_per_view != 0) throw_error("%s: R = %d is not a whole number of views of %d rays", who, R, rays_per_view);
        if (rays_per_view % row_rays != 0) throw_error("%s: rays_per_view = %d is not a whole number of rows of %d rays", who, rays_per_view, row_rays);
        const int V = R / rays_per_view;
        if (V > 65535) throw_error("%s: %d views (at most 65535)", who, V);
        if (R == 0) return;
        if (beta < 2e-3f) beta = 2e-3f; // sdf_activation's clamp, as vanerf_volume_render applies it (a handle's device copy is clamped already)
        VolGrid G;
        for (int a = 0; a < 3; ++a) { G.o[a] = origin[a]; G.s[a] = spacing[a]; }
        G.nx = nx; G.ny = ny; G.nz = nz;
        const int rows = rays_per_view / row_rays;
        const dim3 blocks((unsigned)(((row_rays + PW_TX - 1) / PW_TX) * ((rows + PW_TY - 1) / PW_TY)), (unsigned)V);
        hipLaunchKernelGGL(volume_render_posed_kernel, blocks, dim3(64 * PW_WAVES), 0, (hipStream_t)stream, reinterpret_cast<const float4*>(voxels), G,
                           beta, w ? w->dev_beta : nullptr, rays_d, cam_pos, z, hit, rays_per_view, row_rays, S, reinterpret_cast<const float4*>(T), nf, face,
                           sdf, reach, color, depth, alpha);
        HIP_CHECK(hipGetLastError());
    });
}
