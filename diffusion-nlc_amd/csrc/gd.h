// Gradient-descent constraint projection (affine_proj_GD, image_sample.py:344-357, set up at :384-399): what restore.hip
// (nlc_group_gd) and constraint.hip (nlc_inpaint_gd) share.
//   n_iter steps of  X <- X - lr * grad_X sum_b ||A X_b - y_b||_p ,  p = 1 or 2.
// With r_b = A x_b - y_b the gradient is A^T sign(r_b) (l1, sign(0) = 0) or A^T r_b / ||r_b||_2 (l2, 0 where the norm is 0), and
// every operator here has A A^T = s2 I (s2 = sum_i w_i^2 of one group; 1 for inpainting).  With c = lr * s2 the residual obeys
// a scalar recurrence and x follows it:
//   l1, per group:   r^k   = r^0 - c m_k ,     m_k = sum_{j<k} sign(r^j) ,     x_i^n = x_i^0 - lr w_i m_n
//   l2, per sample:  rho_k = rho_0 - c M_k ,   M_k = sum_{j<k} sign(rho_j) ,   x_i^n = x_i^0 - lr w_i (r_g^0 / rho_0) M_n ,
//                    rho_0 = ||r_b^0||_2  (r^k = (rho_k / rho_0) r^0: the direction never changes, only its sign and length)
// m and M are small integers, so r^k / rho_k are ONE rounded fused multiply-add away from r^0 / rho_0 at every k: no error builds
// up over the iterations.  l1 is local to a group: one launch, one read and one write of x0.  l2 is one per-sample reduction
// (workgroup partials of sum r_g^2, in double, added in a fixed order: no floating-point atomics, bit-reproducible) plus one
// apply pass, whatever n_iter is.
// The structure of those passes stands here once: gd_pass is the device side (one sample per blockIdx.y, a grid-stride walk over
// its items, the l2 partials and scale around it), gd_run the host side (which phases are launched, in which order).  An entry
// point supplies what one item is - a group of restore.hip, a masked float4 / scalar of constraint.hip - and how a phase is launched.
#pragma once
#include "common.h"
#include <cmath>
#include <type_traits>

enum { GD_L1 = 0, GD_L2_SUM = 1, GD_L2_APPLY = 2 };
constexpr int GD_NT = 256;            // threads per workgroup of every GD kernel
constexpr int GD_MAX_GRID = 1024;     // workgroups per sample at most (grid-stride beyond): the partials of one sample

struct gd_params {
    float lr;
    float c;              // float(lr * s2), l1
    double c64;           // lr * s2, l2
    int n_iter;
    double* partials;     // l2: [B][gridDim.x]
};

static inline int gd_grid(int64_t items) {
    const int g = cdiv(items, GD_NT);
    return g > GD_MAX_GRID ? GD_MAX_GRID : (g < 1 ? 1 : g);
}

// validation common to the two entry points; sets the error itself
static inline int gd_check(const char* name, float lr, int n_iter, int loss, const void* workspace) {
    NLC_REQUIRE(loss == 1 || loss == 2, "%s: loss = %d, expected 1 (l1) or 2 (l2)", name, loss);
    NLC_REQUIRE(n_iter >= 0 && n_iter <= 1024, "%s: n_iter = %d outside 0..1024", name, n_iter);
    NLC_REQUIRE(std::isfinite(lr), "%s: lr is not finite", name);
    NLC_REQUIRE(loss == 1 || workspace, "%s: l2 needs a workspace of nlc_gd_workspace_bytes() bytes, got null", name);
    NLC_REQUIRE(((uintptr_t)workspace % 8) == 0, "%s: workspace is not 8-byte aligned", name);
    return NLC_OK;
}

// m_n = sum_{k<n} sign(r^k),  r^k = r0 - c m_k
__device__ __forceinline__ float gd_l1_steps(float r0, float c, int n_iter) {
    float m = 0.f, r = r0;
    for (int k = 0; k < n_iter; ++k) {
        m += (r > 0.f ? 1.f : 0.f) - (r < 0.f ? 1.f : 0.f);
        r = __fmaf_rn(-c, m, r0);
    }
    return m;
}

// the sum of one value per thread over the workgroup, the same bits in every thread: xor butterfly inside a wave, then the
// GD_NT / 64 wave totals in wave order.  `sh`: GD_NT / 64 doubles of LDS.
__device__ __forceinline__ double gd_block_sum(double v, double* sh) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                                   // sh may still be read from a previous call
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = sh[0];
#pragma unroll
    for (int i = 1; i < GD_NT / 64; ++i) t += sh[i];
    return t;
}

// l2 apply: q = lr M_n / rho_0 of this sample (0 where rho_0 is 0 or not a number), from the `nparts` partials of sum r_g^2
__device__ __forceinline__ float gd_l2_scale(const double* parts, int nparts, const gd_params& g, double* sh) {
    double t = 0.0;
    for (int i = threadIdx.x; i < nparts; i += GD_NT) t += parts[i];
    t = gd_block_sum(t, sh);
    const double rho0 = sqrt(t);
    if (!(rho0 > 0.0) || isinf(rho0)) return 0.f;      // uniform over the workgroup: t is
    double m = 0.0, rho = rho0;
    for (int k = 0; k < g.n_iter; ++k) {
        m += (rho > 0.0 ? 1.0 : 0.0) - (rho < 0.0 ? 1.0 : 0.0);
        rho = fma(-g.c64, m, rho0);
    }
    return (float)((double)g.lr * m / rho0);
}

// One phase over the `items` of sample blockIdx.y, gridDim.x workgroups of GD_NT threads striding over them.  body(i, q, acc) does
// item i: GD_L1 and GD_L2_APPLY update it (q: gd_l2_scale of this sample, l2 only), GD_L2_SUM adds its squared residuals to the
// thread's `acc`, in double, in the order the thread meets them; the workgroup's total becomes its partial.  A lambda given as
// body carries __attribute__((always_inline)): it is then inlined before it is optimised on its own, and the kernel compiles
// to what the loop written out in place compiles to (otherwise the float4 loads of constraint.hip come out split).
template <int PH, class Body> __device__ __forceinline__ void gd_pass(int64_t items, const gd_params& g, Body body) {
    __shared__ double sh[GD_NT / 64];
    double* parts = g.partials + (int64_t)blockIdx.y * gridDim.x;
    float q = 0.f;
    if constexpr (PH == GD_L2_APPLY) {
        q = gd_l2_scale(parts, gridDim.x, g, sh);
        if (q == 0.f) return;                          // rho_0 = 0 or M_n = 0: the sample stays as it is
    }
    double acc = 0.0;
    for (int64_t i = (int64_t)blockIdx.x * GD_NT + threadIdx.x; i < items; i += (int64_t)gridDim.x * GD_NT) body(i, q, acc);
    if constexpr (PH == GD_L2_SUM) {
        acc = gd_block_sum(acc, sh);
        if (threadIdx.x == 0) parts[blockIdx.x] = acc;
    }
}

// The launches of one projection: l1 is one pass; l2 is the pass that sums, then the pass that applies.  launch(phase) enqueues
// the kernel of one phase, given as std::integral_constant.  Sets the error itself.
template <class Launch> int gd_run(const char* name, int loss, Launch launch) {
    if (loss == 1) {
        launch(std::integral_constant<int, GD_L1>{});
    } else {
        launch(std::integral_constant<int, GD_L2_SUM>{});
        NLC_CHECK_LAUNCH(name);
        launch(std::integral_constant<int, GD_L2_APPLY>{});
    }
    NLC_CHECK_LAUNCH(name);
    return NLC_OK;
}
