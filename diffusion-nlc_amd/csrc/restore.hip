// Group-sum measurement operators on the NCHW f32 sampler state: average-pooling super-resolution and colorization.
// functions/svd_operators.py:479-533 (SuperResolution) and :627-667 (Colorization) reach "one weighted sum per group of n
// entries" through unfold / permute / strided-scatter chains and a batched 1 x n matmul with an SVD factor.  In closed form, with
// the group's weights w (n entries) and p_i = w_i / sum_j w_j^2:
//   A(x)[group]        = sum_i w_i x_i
//   A^+(y)[i of group] = p_i y[group]
//   x0 - A^+(A x0 - y) = x0_i + p_i (y[group] - sum_j w_j x0_j)            (affine_svd, image_sample.py:376-380)
// BLOCK mode: a group is an r x r spatial block of one channel, i runs row-major inside the block, y is [b][c][by][bx]
// (SuperResolution.Vt, :515).  CHANNEL mode: a group is the 3 channels of one pixel, y is [b][p].
// One thread per group; the sum runs i = 0 .. n-1 as separately rounded products and additions, the update of the projection is
// one fused multiply-add.  Bandwidth-bound: no LDS, no MFMA.  Adjacent threads take adjacent blocks of one block-row, so a
// wavefront's row loads are contiguous; with r = 2 / 4 / 8 and a 16-byte aligned tensor a row is one float2 / float4 / two float4.
// nlc_group_gd (affine_proj_GD, image_sample.py:344-357,384-399) walks the groups the same way; its closed forms are in gd.h.
#include "common.h"
#include "gd.h"

namespace {
constexpr int NT = 256;
enum { OP_A = 0, OP_APINV = 1, OP_PROJECT = 2 };

template <int R, bool VEC> __device__ __forceinline__ void load_row(const float* p, float* v) {
    if constexpr (VEC && R == 2) {
        const float2 t = *reinterpret_cast<const float2*>(p);
        v[0] = t.x; v[1] = t.y;
    } else if constexpr (VEC && (R == 4 || R == 8)) {
#pragma unroll
        for (int k = 0; k < R; k += 4) {
            const float4 t = *reinterpret_cast<const float4*>(p + k);
            v[k] = t.x; v[k + 1] = t.y; v[k + 2] = t.z; v[k + 3] = t.w;
        }
    } else {
#pragma unroll
        for (int k = 0; k < R; ++k) v[k] = p[k];
    }
}

template <int R, bool VEC> __device__ __forceinline__ void store_row(float* p, const float* v) {
    if constexpr (VEC && R == 2) {
        *reinterpret_cast<float2*>(p) = make_float2(v[0], v[1]);
    } else if constexpr (VEC && (R == 4 || R == 8)) {
#pragma unroll
        for (int k = 0; k < R; k += 4) *reinterpret_cast<float4*>(p + k) = make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
    } else {
#pragma unroll
        for (int k = 0; k < R; ++k) p[k] = v[k];
    }
}

// sum_i w_i v_i, i ascending: n products and n-1 additions, each rounded once (no contraction)
template <int N> __device__ __forceinline__ float group_sum(const float* w, const float* v) {
    float s = __fmul_rn(w[0], v[0]);
#pragma unroll
    for (int i = 1; i < N; ++i) s = __fadd_rn(s, __fmul_rn(w[i], v[i]));
    return s;
}

// x: [B][C][H][W] (read by OP_A, written by OP_APINV, both by OP_PROJECT) ; y: [B][C][H/R][W/R] (written by OP_A, read otherwise)
template <int R, bool VEC, int OP>
__global__ __launch_bounds__(NT) void group_block_kernel(float* x, float* y, const nlc_group_desc d) {
    const int Wb = d.W / R;
    const int64_t G = (int64_t)d.C * (d.H / R) * Wb;             // groups per sample
    const int b = blockIdx.y;
    float* xb = x + (int64_t)b * d.C * d.H * d.W;
    float* yb = y + (int64_t)b * G;
    for (int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x; g < G; g += (int64_t)gridDim.x * NT) {
        const int64_t row = g / Wb;                              // c * (H/R) + by: the block-row, counted over all channels
        const int bx = (int)(g - row * Wb);
        float* base = xb + row * R * d.W + (int64_t)bx * R;
        float v[R * R];
        if constexpr (OP == OP_APINV) {
            const float yg = yb[g];
#pragma unroll
            for (int i = 0; i < R * R; ++i) v[i] = __fmul_rn(d.p[i], yg);
        } else {
#pragma unroll
            for (int j = 0; j < R; ++j) load_row<R, VEC>(base + (int64_t)j * d.W, v + j * R);
            const float s = group_sum<R * R>(d.w, v);
            if constexpr (OP == OP_A) {
                yb[g] = s;
            } else {
                const float r = __fsub_rn(yb[g], s);
#pragma unroll
                for (int i = 0; i < R * R; ++i) v[i] = __fmaf_rn(d.p[i], r, v[i]);
            }
        }
        if constexpr (OP != OP_A) {
#pragma unroll
            for (int j = 0; j < R; ++j) store_row<R, VEC>(base + (int64_t)j * d.W, v + j * R);
        }
    }
}

// x: [B][3][HW] ; y: [B][HW]
template <int OP>
__global__ __launch_bounds__(NT) void group_channel_kernel(float* x, float* y, const nlc_group_desc d) {
    const int64_t HW = (int64_t)d.H * d.W;
    const int b = blockIdx.y;
    float* xb = x + (int64_t)b * 3 * HW;
    float* yb = y + (int64_t)b * HW;
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < HW; p += (int64_t)gridDim.x * NT) {
        float v[3];
        if constexpr (OP == OP_APINV) {
            const float yg = yb[p];
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = __fmul_rn(d.p[c], yg);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c) v[c] = xb[c * HW + p];
            const float s = group_sum<3>(d.w, v);
            if constexpr (OP == OP_A) {
                yb[p] = s;
            } else {
                const float r = __fsub_rn(yb[p], s);
#pragma unroll
                for (int c = 0; c < 3; ++c) v[c] = __fmaf_rn(d.p[c], r, v[c]);
            }
        }
        if constexpr (OP != OP_A) {
#pragma unroll
            for (int c = 0; c < 3; ++c) xb[c * HW + p] = v[c];
        }
    }
}

template <int R, int OP>
void launch_block(float* x, float* y, const nlc_group_desc& d, dim3 grid, hipStream_t s) {
    // a row of R floats starts at a multiple of R floats from the tensor's base (W % R == 0): aligned iff the base is
    constexpr bool kCanVec = R == 2 || R == 4 || R == 8;
    const uintptr_t align = R == 2 ? 8 : 16;
    if (kCanVec && ((uintptr_t)x % align) == 0)
        hipLaunchKernelGGL((group_block_kernel<R, kCanVec, OP>), grid, dim3(NT), 0, s, x, y, d);
    else
        hipLaunchKernelGGL((group_block_kernel<R, false, OP>), grid, dim3(NT), 0, s, x, y, d);
}

// the rules every entry point holds a descriptor to; sets the error itself
int check_group_desc(const nlc_group_desc& d, const char* name) {
    NLC_REQUIRE(d.mode == NLC_GROUP_BLOCK || d.mode == NLC_GROUP_CHANNEL, "%s: unknown mode %d", name, d.mode);
    NLC_REQUIRE(d.B > 0 && d.B <= 65535, "%s: B = %d outside 1..65535", name, d.B);
    NLC_REQUIRE(d.C > 0 && d.H > 0 && d.W > 0, "%s: bad shape C=%d H=%d W=%d", name, d.C, d.H, d.W);
    NLC_REQUIRE(d.r >= 1 && d.r <= 8, "%s: r = %d outside 1..8", name, d.r);
    if (d.mode == NLC_GROUP_CHANNEL)
        NLC_REQUIRE(d.C == 3, "%s: CHANNEL mode needs C = 3, got %d", name, d.C);
    else
        NLC_REQUIRE(d.H % d.r == 0 && d.W % d.r == 0, "%s: H=%d W=%d are not multiples of r=%d", name, d.H, d.W, d.r);
    return NLC_OK;
}

template <int OP>
int launch_group(float* x, float* y, const nlc_group_desc& d, void* stream, const char* name) {
    NLC_REQUIRE(x && y, "%s: null pointer", name);
    NLC_TRY(check_group_desc(d, name));
    hipStream_t s = (hipStream_t)stream;
    if (d.mode == NLC_GROUP_CHANNEL) {
        int g = cdiv((int64_t)d.H * d.W, NT); if (g > 1024) g = 1024;
        hipLaunchKernelGGL((group_channel_kernel<OP>), dim3(g, d.B), dim3(NT), 0, s, x, y, d);
    } else {
        int g = cdiv((int64_t)d.C * (d.H / d.r) * (d.W / d.r), NT); if (g > 1024) g = 1024;
        const dim3 grid(g, d.B);
        switch (d.r) {
            case 1: launch_block<1, OP>(x, y, d, grid, s); break;
            case 2: launch_block<2, OP>(x, y, d, grid, s); break;
            case 3: launch_block<3, OP>(x, y, d, grid, s); break;
            case 4: launch_block<4, OP>(x, y, d, grid, s); break;
            case 5: launch_block<5, OP>(x, y, d, grid, s); break;
            case 6: launch_block<6, OP>(x, y, d, grid, s); break;
            case 7: launch_block<7, OP>(x, y, d, grid, s); break;
            default: launch_block<8, OP>(x, y, d, grid, s); break;
        }
    }
    NLC_CHECK_LAUNCH(name);
    return NLC_OK;
}

// ---- gradient-descent projection (gd.h).  v: the N entries of one group, yg its measurement.  GD_L2_SUM returns r^2 in double
//      and leaves v alone; GD_L1 / GD_L2_APPLY update v (q: the sample's lr M_n / rho_0, l2 only). ------------------------------------
template <int N, int PH>
__device__ __forceinline__ double gd_group(float* v, float yg, const float* w, const gd_params& g, float q) {
    const float r = __fsub_rn(group_sum<N>(w, v), yg);
    if constexpr (PH == GD_L2_SUM) {
        return (double)r * (double)r;
    } else {
        // x_i <- x_i - w_i a:  a = lr m_n (l1) or q r_g (l2), rounded once; the update is one fused multiply-add
        const float a = PH == GD_L1 ? __fmul_rn(g.lr, gd_l1_steps(r, g.c, g.n_iter)) : __fmul_rn(q, r);
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = __fmaf_rn(-w[i], a, v[i]);
        return 0.0;
    }
}

template <int R, bool VEC, int PH>
__global__ __launch_bounds__(NT) void group_block_gd_kernel(float* x, const float* y, const nlc_group_desc d, const gd_params g) {
    __shared__ double sh[NT / 64];
    const int Wb = d.W / R;
    const int64_t G = (int64_t)d.C * (d.H / R) * Wb;
    const int b = blockIdx.y;
    float* xb = x + (int64_t)b * d.C * d.H * d.W;
    const float* yb = y + (int64_t)b * G;
    double* parts = g.partials + (int64_t)b * gridDim.x;
    float q = 0.f;
    if constexpr (PH == GD_L2_APPLY) {
        q = gd_l2_scale(parts, gridDim.x, g, sh);
        if (q == 0.f) return;                                               // rho_0 = 0 or M_n = 0: the sample stays as it is
    }
    double acc = 0.0;
    for (int64_t gi = (int64_t)blockIdx.x * NT + threadIdx.x; gi < G; gi += (int64_t)gridDim.x * NT) {
        const int64_t row = gi / Wb;
        const int bx = (int)(gi - row * Wb);
        float* base = xb + row * R * d.W + (int64_t)bx * R;
        float v[R * R];
#pragma unroll
        for (int j = 0; j < R; ++j) load_row<R, VEC>(base + (int64_t)j * d.W, v + j * R);
        acc += gd_group<R * R, PH>(v, yb[gi], d.w, g, q);
        if constexpr (PH != GD_L2_SUM) {
#pragma unroll
            for (int j = 0; j < R; ++j) store_row<R, VEC>(base + (int64_t)j * d.W, v + j * R);
        }
    }
    if constexpr (PH == GD_L2_SUM) {
        acc = gd_block_sum(acc, sh);
        if (threadIdx.x == 0) parts[blockIdx.x] = acc;
    }
}

template <int PH>
__global__ __launch_bounds__(NT) void group_channel_gd_kernel(float* x, const float* y, const nlc_group_desc d, const gd_params g) {
    __shared__ double sh[NT / 64];
    const int64_t HW = (int64_t)d.H * d.W;
    const int b = blockIdx.y;
    float* xb = x + (int64_t)b * 3 * HW;
    const float* yb = y + (int64_t)b * HW;
    double* parts = g.partials + (int64_t)b * gridDim.x;
    float q = 0.f;
    if constexpr (PH == GD_L2_APPLY) {
        q = gd_l2_scale(parts, gridDim.x, g, sh);
        if (q == 0.f) return;
    }
    double acc = 0.0;
    for (int64_t p = (int64_t)blockIdx.x * NT + threadIdx.x; p < HW; p += (int64_t)gridDim.x * NT) {
        float v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = xb[c * HW + p];
        acc += gd_group<3, PH>(v, yb[p], d.w, g, q);
        if constexpr (PH != GD_L2_SUM) {
#pragma unroll
            for (int c = 0; c < 3; ++c) xb[c * HW + p] = v[c];
        }
    }
    if constexpr (PH == GD_L2_SUM) {
        acc = gd_block_sum(acc, sh);
        if (threadIdx.x == 0) parts[blockIdx.x] = acc;
    }
}

template <int R, int PH>
void launch_block_gd(float* x, const float* y, const nlc_group_desc& d, const gd_params& g, dim3 grid, hipStream_t s) {
    constexpr bool kCanVec = R == 2 || R == 4 || R == 8;                    // as launch_block
    const uintptr_t align = R == 2 ? 8 : 16;
    if (kCanVec && ((uintptr_t)x % align) == 0)
        hipLaunchKernelGGL((group_block_gd_kernel<R, kCanVec, PH>), grid, dim3(NT), 0, s, x, y, d, g);
    else
        hipLaunchKernelGGL((group_block_gd_kernel<R, false, PH>), grid, dim3(NT), 0, s, x, y, d, g);
}

template <int PH>
void launch_gd(float* x, const float* y, const nlc_group_desc& d, const gd_params& g, hipStream_t s) {
    if (d.mode == NLC_GROUP_CHANNEL) {
        hipLaunchKernelGGL((group_channel_gd_kernel<PH>), dim3(gd_grid((int64_t)d.H * d.W), d.B), dim3(NT), 0, s, x, y, d, g);
        return;
    }
    const dim3 grid(gd_grid((int64_t)d.C * (d.H / d.r) * (d.W / d.r)), d.B);
    switch (d.r) {
        case 1: launch_block_gd<1, PH>(x, y, d, g, grid, s); break;
        case 2: launch_block_gd<2, PH>(x, y, d, g, grid, s); break;
        case 3: launch_block_gd<3, PH>(x, y, d, g, grid, s); break;
        case 4: launch_block_gd<4, PH>(x, y, d, g, grid, s); break;
        case 5: launch_block_gd<5, PH>(x, y, d, g, grid, s); break;
        case 6: launch_block_gd<6, PH>(x, y, d, g, grid, s); break;
        case 7: launch_block_gd<7, PH>(x, y, d, g, grid, s); break;
        default: launch_block_gd<8, PH>(x, y, d, g, grid, s); break;
    }
}
}  // namespace

extern "C" int nlc_group_A(const float* x, nlc_group_desc desc, float* y_out, void* stream) {
    return launch_group<OP_A>(const_cast<float*>(x), y_out, desc, stream, "nlc_group_A");
}

extern "C" int nlc_group_Apinv(const float* y, nlc_group_desc desc, float* x_out, void* stream) {
    return launch_group<OP_APINV>(x_out, const_cast<float*>(y), desc, stream, "nlc_group_Apinv");
}

extern "C" int nlc_group_project(float* x0, const float* y, nlc_group_desc desc, void* stream) {
    return launch_group<OP_PROJECT>(x0, const_cast<float*>(y), desc, stream, "nlc_group_project");
}

extern "C" int64_t nlc_gd_workspace_bytes(int B, int64_t entries_per_sample) {
    if (B <= 0 || entries_per_sample <= 0) return 0;
    return (int64_t)B * gd_grid(entries_per_sample) * (int64_t)sizeof(double);
}

extern "C" int nlc_group_gd(float* x0, const float* y, nlc_group_desc desc, float lr, int n_iter, int loss, void* workspace,
                            void* stream) {
    static_assert(NT == GD_NT, "the GD helpers reduce over GD_NT threads");
    const char* name = "nlc_group_gd";
    NLC_REQUIRE(x0 && y, "%s: null pointer", name);
    NLC_TRY(check_group_desc(desc, name));
    NLC_TRY(gd_check(name, lr, n_iter, loss, workspace));
    if (n_iter == 0) return NLC_OK;
    const int n = desc.mode == NLC_GROUP_CHANNEL ? 3 : desc.r * desc.r;
    double s2 = 0.0;                                                        // A A^T = s2 I
    for (int i = 0; i < n; ++i) s2 += (double)desc.w[i] * (double)desc.w[i];
    NLC_REQUIRE(std::isfinite(lr * (float)n_iter) && std::isfinite((float)((double)lr * s2)),
                "%s: lr * n_iter or lr * sum w^2 overflows float (lr = %g)", name, (double)lr);
    gd_params g{lr, (float)((double)lr * s2), (double)lr * s2, n_iter, (double*)workspace};
    hipStream_t s = (hipStream_t)stream;
    if (loss == 1) {
        launch_gd<GD_L1>(x0, y, desc, g, s);
    } else {
        launch_gd<GD_L2_SUM>(x0, y, desc, g, s);
        NLC_CHECK_LAUNCH(name);
        launch_gd<GD_L2_APPLY>(x0, y, desc, g, s);
    }
    NLC_CHECK_LAUNCH(name);
    return NLC_OK;
}
