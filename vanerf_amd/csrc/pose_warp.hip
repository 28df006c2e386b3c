// pose_warp.hip -- the baked volume rendered in another pose of the same mesh (the comments of vanerf_pose_transforms /
// vanerf_volume_render_posed in the header).  The volume is a field in the SOURCE pose's space and the mesh has the same faces in every pose,
// so a sample of a ray through the POSED hand is carried back into source space by the affine map of its closest face and looked up there:
// no network per view, and the only per-sample geometry work is the mesh query the library already has, whose outputs (face, sdf) this file
// takes as inputs.  A preview under the usual surface-aligned deformation model, not what the networks would render from a photograph of the
// new pose.  The restatement the tests hold these kernels to is the numpy code of tests/test_posed_volume_cpu.py.
//
// The march is volume_render_kernel's (volume_render.hip) with another sample functor: wave_ray.h's march_rounds on volume_field.h's
// field, so the identity pose renders vanerf_volume_render's bits by construction.  New per lane and round: the coalesced loads of face and sdf, three 16-byte loads of the face's record and nine multiplies.  The table of records (nf x 48 bytes,
// 149 KB for the two-hand mesh) stays in L2 and is shared by every wave; it is NOT staged in LDS, which it would fill, taking the occupancy
// that hides the gathers.  No atomics, no device-side state, no LDS.  Built with -ffp-contract=off: every product and sum is its own IEEE
// operation.
#include "common.h"
#include "volume_field.h"
#include "wave_ray.h"

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

#ifdef VANERF_POSED_NO_SKIP
constexpr bool PW_SKIP = false;
#else
constexpr bool PW_SKIP = true;
#endif

// volume_render_kernel with the sample carried into source space first.  A sample is EMPTY (c = 0) iff face < 0, face >= nf, sdf is not
// finite or sdf > reach; the others are carried to q = A p + t by their face's record and interpolated there.  SKIP: a round all of whose
// samples are empty -- most of a ray is farther than `reach` from the hand -- issues no gather; the bits are the same either way, an empty
// sample has c = 0 with or without the branch (a build with -DVANERF_POSED_NO_SKIP takes it out, to show that and to time it:
// tools/perf_posed.py).
__global__ __launch_bounds__(64 * RAY_WAVES) void volume_render_posed_kernel(const float4* __restrict__ voxels, const VolGrid G, float beta,
                                                                             const float* __restrict__ beta_dev, const float* __restrict__ rays_d,
                                                                             const float* __restrict__ cam_pos, const float* __restrict__ z,
                                                                             const uint8_t* __restrict__ hit, int rays_per_view, int row_rays, int S,
                                                                             const float4* __restrict__ T, int nf, const int32_t* __restrict__ face,
                                                                             const float* __restrict__ sdf, float reach, float* __restrict__ color,
                                                                             float* __restrict__ depth, float* __restrict__ alpha)
{
    const int lane = threadIdx.x & 63;
    int v;
    size_t r;
    if (!march_ray(hit, rays_per_view, row_rays, lane, color, depth, alpha, v, r)) return; // whole wave
    if (beta_dev) beta = *beta_dev; // a weight handle's device copy of sigmoid_beta, already clamped
    const float ox = cam_pos[4 * v], oy = cam_pos[4 * v + 1], oz = cam_pos[4 * v + 2];
    const float dx = rays_d[3 * r], dy = rays_d[3 * r + 1], dz = rays_d[3 * r + 2];
    const float* zr = z + r * (size_t)S;
    const int32_t* fr = face + r * (size_t)S;
    const float* sr = sdf + r * (size_t)S;
    const RaySums<false> sums = march_rounds(zr, S, lane, [&](int i, float zi, float& c, float4& q) {
        int fi = -1;
        float sd = 0.0f;
        if (i < S) { fi = fr[i]; sd = sr[i]; }
        const bool live = fi >= 0 && fi < nf && fabsf(sd) <= FLT_MAX && sd <= reach; // (NaN compares false)
        if (PW_SKIP && __ballot(live) == 0ull) return; // wave-uniform
        if (!live) return;
        const float dist = sample_dist(zr, i, S, zi);
        const float4* t = T + 3 * (size_t)fi;
        const float4 t0 = t[0], t1 = t[1], t2 = t[2]; // A00 A01 A02 A10 | A11 A12 A20 A21 | A22 tx ty tz
        const float ppx = ox + dx * zi, ppy = oy + dy * zi, ppz = oz + dz * zi; // p = o + d z per axis: sample_points_kernel's expression
        const float qx = ((t0.x * ppx + t0.y * ppy) + t0.z * ppz) + t2.y;
        const float qy = ((t0.w * ppx + t1.x * ppy) + t1.y * ppz) + t2.z;
        const float qz = ((t1.z * ppx + t1.w * ppy) + t2.x * ppz) + t2.w;
        q = field_at_point(voxels, G, qx, qy, qz);
        const float sg = sdf_sigmoid(q.x, beta) / beta;
        c = 1.0f - expf(-sg * dist);
    });
    if (lane == 0) sums.store(color, depth, alpha, nullptr, r);
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
        beta = check_beta(who, w, beta);
        const int V = check_ray_grid(who, R, rays_per_view, row_rays);
        if (R == 0) return;
        hipLaunchKernelGGL(volume_render_posed_kernel, tile_blocks(row_rays, rays_per_view / row_rays, V), dim3(64 * RAY_WAVES), 0, (hipStream_t)stream,
                           reinterpret_cast<const float4*>(voxels), make_grid(origin, spacing, nx, ny, nz), beta, w ? w->dev_beta : nullptr, rays_d, cam_pos, z,
                           hit, rays_per_view, row_rays, S, reinterpret_cast<const float4*>(T), nf, face, sdf, reach, color, depth, alpha);
        HIP_CHECK(hipGetLastError());
    });
}
