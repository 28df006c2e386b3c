// mano_joint_forward.h -- the fp64 joint chain that mano_skin_backward.hip and mano_skin_normal.hip both recompute: device code, one copy.
#pragma once
#include "mano_tables.h"

#include <cmath>

namespace vanerf {
namespace mano {

// Steps 1, 3, 5 and J of step 2 for one pose, by one wave: the arithmetic of mano_joint_kernel, operation for operation.  Leaves the full
// axis-angle (sr), R, J and G in LDS; A and the pose feature go to `A` / `pf` (fp32) when given.  Ends behind a barrier.
__device__ __forceinline__ void joint_forward(const ManoTables& t, int nj, int nb, const float* __restrict__ pose, const float* __restrict__ betas,
                                              int flat_hand_mean, int lane, double (*sr)[3], double (*sR)[9], double (*sJ)[3], double (*sG)[12],
                                              float* __restrict__ A, float* __restrict__ pf)
{
    if (lane < nj) {
        double r[3];
        for (int k = 0; k < 3; ++k) {
            r[k] = (double)pose[3 * lane + k] + (flat_hand_mean ? 0.0 : t.hm[3 * lane + k]);
            sr[lane][k] = r[k];
        }
        const double e0 = r[0] + 1e-8, e1 = r[1] + 1e-8, e2 = r[2] + 1e-8;
        const double angle = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
        const double dx = r[0] / angle, dy = r[1] / angle, dz = r[2] / angle;
        const double s = sin(angle), c1 = 1.0 - cos(angle);
        double m[9];
        m[0] = c1 * -(dz * dz + dy * dy);
        m[1] = s * -dz + c1 * (dx * dy);
        m[2] = s * dy + c1 * (dx * dz);
        m[3] = s * dz + c1 * (dx * dy);
        m[4] = c1 * -(dz * dz + dx * dx);
        m[5] = s * -dx + c1 * (dy * dz);
        m[6] = s * -dy + c1 * (dx * dz);
        m[7] = s * dx + c1 * (dy * dz);
        m[8] = c1 * -(dx * dx + dy * dy);
        for (int e = 0; e < 9; ++e) {
            sR[lane][e] = (e % 4 == 0 ? 1.0 : 0.0) + m[e];
            if (pf && lane >= 1) pf[(lane - 1) * 9 + e] = (float)m[e];
        }
        for (int k = 0; k < 3; ++k) {
            double sum = 0.0;
            for (int b = 0; b < nb; ++b) sum = sum + t.Js[(lane * 3 + k) * nb + b] * (double)betas[b];
            sJ[lane][k] = t.Jt[lane * 3 + k] + sum;
        }
    }
    __syncthreads();
    const int row = (lane >> 2) % 3, col = lane & 3;
    for (int j = 0; j < nj; ++j) {
        if (lane < 12) {
            double g;
            if (j == 0) {
                g = col < 3 ? sR[0][row * 3 + col] : sJ[0][row];
            } else {
                int par = t.parents[j];
                par = par < 0 ? 0 : (par > j - 1 ? j - 1 : par); // (checked at the pack; a foreign buffer must not index outside the block's LDS)
                const double* G = sG[par];
                double l0, l1, l2;
                if (col < 3) { l0 = sR[j][col]; l1 = sR[j][3 + col]; l2 = sR[j][6 + col]; }
                else { l0 = sJ[j][0] - sJ[par][0]; l1 = sJ[j][1] - sJ[par][1]; l2 = sJ[j][2] - sJ[par][2]; }
                g = (G[row * 4] * l0 + G[row * 4 + 1] * l1) + G[row * 4 + 2] * l2;
                if (col == 3) g = g + G[row * 4 + 3];
            }
            sG[j][row * 4 + col] = g;
        }
        __syncthreads();
    }
    if (A && lane < nj) {
        const double* G = sG[lane];
        for (int k = 0; k < 3; ++k) {
            for (int c = 0; c < 3; ++c) A[lane * 12 + k * 4 + c] = (float)G[k * 4 + c];
            A[lane * 12 + k * 4 + 3] = (float)(G[k * 4 + 3] - ((G[k * 4] * sJ[lane][0] + G[k * 4 + 1] * sJ[lane][1]) + G[k * 4 + 2] * sJ[lane][2]));
        }
    }
}

} // namespace mano
} // namespace vanerf
