// Inpainting measurement operator on the NCHW f32 sampler state.
// functions/svd_operators.py:324-359 expresses A and A^+ as permute / index_select / scatter chains over
// a pixel-interleaved (H*W, C) flattening; both are pure gathers:
//   A(x)[b][j]          = x[b][c][p]            with kept[j] = p*C + c
//   A_pinv(y)[b][c][p]  = inv[p*C + c] >= 0 ? y[b][inv[p*C + c]] : 0
// The per-step projection  x0 <- x0 - A^+(A x0 - y)  ("copy the known pixels") is fused into
// nlc_sched_step (mask / known), so these two kernels run once per batch.
// nlc_inpaint_gd is the gradient-descent projection (affine_proj_GD, image_sample.py:344-357,384-399) over the same mask / known
// pair.  Its closed forms, the phases of a pass and their launch order are in gd.h; this file says what one item of a pass is.
#include "common.h"
#include "gd.h"

namespace {
constexpr int NT = 256;

__global__ void inpaint_A_kernel(const float* __restrict__ x, const int64_t* __restrict__ kept, float* __restrict__ out,
                                 int64_t nk, int C, int64_t HW) {
    const int b = blockIdx.y;
    for (int64_t j = (int64_t)blockIdx.x * NT + threadIdx.x; j < nk; j += (int64_t)gridDim.x * NT) {
        const int64_t idx = kept[j];
        const int64_t p = idx / C; const int c = (int)(idx - p * C);
        out[(int64_t)b * nk + j] = x[((int64_t)b * C + c) * HW + p];
    }
}

__global__ void inpaint_Apinv_kernel(const float* __restrict__ y, const int32_t* __restrict__ inv, float* __restrict__ out,
                                     int64_t nk, int C, int64_t HW) {
    const int b = blockIdx.y;
    const int64_t n = (int64_t)C * HW;
    for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT) {
        const int c = (int)(i / HW); const int64_t p = i - (int64_t)c * HW;
        const int32_t j = inv[p * C + c];
        out[(int64_t)b * n + i] = j >= 0 ? y[(int64_t)b * nk + j] : 0.f;
    }
}

// Gradient-descent projection with A = "keep the known entries": s2 = 1, the residual of a known entry is x - known, a missing
// entry has none and never moves.  x: [B][n], mask / known: [n] / [B][n], n = C*HW.  An item of the pass (gd_pass, gd.h) is V
// entries: V = 4: float4 items (n % 4 == 0 and all three bases 16-byte aligned), V = 1: scalar.
template <int V, int PH>
__global__ __launch_bounds__(NT) void inpaint_gd_kernel(float* x, const float* __restrict__ mask, const float* __restrict__ known,
                                                        int64_t n, const gd_params g) {
    float* xb = x + (int64_t)blockIdx.y * n;
    const float* kb = known + (int64_t)blockIdx.y * n;
    gd_pass<PH>(n / V, g, [&](int64_t i, float q, double& acc) __attribute__((always_inline)) {
        float v[V], m[V], k[V];
        if constexpr (V == 4) {
            const float4 tv = reinterpret_cast<const float4*>(xb)[i], tm = reinterpret_cast<const float4*>(mask)[i],
                         tk = reinterpret_cast<const float4*>(kb)[i];
            v[0] = tv.x; v[1] = tv.y; v[2] = tv.z; v[3] = tv.w;
            m[0] = tm.x; m[1] = tm.y; m[2] = tm.z; m[3] = tm.w;
            k[0] = tk.x; k[1] = tk.y; k[2] = tk.z; k[3] = tk.w;
        } else {
            v[0] = xb[i]; m[0] = mask[i]; k[0] = kb[i];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float r = m[j] != 0.f ? __fsub_rn(v[j], k[j]) : 0.f;
            if constexpr (PH == GD_L2_SUM) acc += (double)r * (double)r;
            else if constexpr (PH == GD_L1) v[j] = __fmaf_rn(-g.lr, gd_l1_steps(r, g.c, g.n_iter), v[j]);
            else v[j] = __fmaf_rn(-q, r, v[j]);
        }
        if constexpr (PH != GD_L2_SUM) {
            if constexpr (V == 4) reinterpret_cast<float4*>(xb)[i] = make_float4(v[0], v[1], v[2], v[3]);
            else xb[i] = v[0];
        }
    });
}
}  // namespace

extern "C" int nlc_inpaint_gd(float* x0, const float* mask_chw, const float* known, int B, int C, int HW, float lr, int n_iter,
                              int loss, void* workspace, void* stream) {
    static_assert(NT == GD_NT, "the GD helpers reduce over GD_NT threads");
    const char* name = "nlc_inpaint_gd";
    NLC_REQUIRE(x0 && mask_chw && known, "%s: null pointer", name);
    NLC_REQUIRE(B > 0 && B <= 65535 && C > 0 && HW > 0, "%s: bad shape B=%d C=%d HW=%d", name, B, C, HW);
    NLC_TRY(gd_check(name, lr, n_iter, loss, workspace));
    if (n_iter == 0) return NLC_OK;
    const gd_params g{lr, lr, (double)lr, n_iter, (double*)workspace};
    const int64_t n = (int64_t)C * HW;
    const bool vec = n % 4 == 0 && (((uintptr_t)x0 | (uintptr_t)mask_chw | (uintptr_t)known) % 16) == 0;
    const dim3 grid(gd_grid(vec ? n / 4 : n), B);
    return gd_run(name, loss, [&](auto ph) {
        if (vec) hipLaunchKernelGGL((inpaint_gd_kernel<4, ph()>), grid, dim3(NT), 0, (hipStream_t)stream, x0, mask_chw, known, n, g);
        else hipLaunchKernelGGL((inpaint_gd_kernel<1, ph()>), grid, dim3(NT), 0, (hipStream_t)stream, x0, mask_chw, known, n, g);
    });
}

extern "C" int nlc_inpaint_A(const float* x, const int64_t* kept, float* out, int B, int C, int64_t HW, int64_t nk, void* stream) {
    NLC_REQUIRE(x && kept && out && B > 0 && B <= 65535 && C > 0 && HW > 0 && nk > 0, "nlc_inpaint_A: bad arguments");
    int g = cdiv(nk, NT); if (g > 1024) g = 1024;
    hipLaunchKernelGGL(inpaint_A_kernel, dim3(g, B), dim3(NT), 0, (hipStream_t)stream, x, kept, out, nk, C, HW);
    NLC_CHECK_LAUNCH("nlc_inpaint_A");
    return NLC_OK;
}

extern "C" int nlc_inpaint_Apinv(const float* y, const int32_t* inv, float* out, int B, int C, int64_t HW, int64_t nk, void* stream) {
    NLC_REQUIRE(y && inv && out && B > 0 && B <= 65535 && C > 0 && HW > 0 && nk > 0, "nlc_inpaint_Apinv: bad arguments");
    int g = cdiv((int64_t)C * HW, NT); if (g > 1024) g = 1024;
    hipLaunchKernelGGL(inpaint_Apinv_kernel, dim3(g, B), dim3(NT), 0, (hipStream_t)stream, y, inv, out, nk, C, HW);
    NLC_CHECK_LAUNCH("nlc_inpaint_Apinv");
    return NLC_OK;
}
