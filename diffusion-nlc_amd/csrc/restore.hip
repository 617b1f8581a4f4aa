// Group-sum measurement operators on the NCHW f32 sampler state: average-pooling super-resolution and colorization.
// functions/svd_operators.py:479-533 (SuperResolution) and :627-667 (Colorization) reach "one weighted sum per group of n
// entries" through unfold / permute / strided-scatter chains and a batched 1 x n matmul with an SVD factor.  In closed form, with
// the group's weights w (n entries) and p_i = w_i / sum_j w_j^2:
//   A(x)[group]        = sum_i w_i x_i
//   A^+(y)[i of group] = p_i y[group]
//   x0 - A^+(A x0 - y) = x0_i + p_i (y[group] - sum_j w_j x0_j)            (affine_svd, image_sample.py:376-380)
// and the gradient-descent projection nlc_group_gd (affine_proj_GD, image_sample.py:344-357,384-399; closed forms in gd.h).
// The file is layout x operation.  A LAYOUT is the only code that knows where a group's entries live: BlockLayout<R, VEC> (an
// r x r spatial block of one channel, i row-major inside the block, y is [b][c][by][bx]: SuperResolution.Vt, :515) and
// ChannelLayout (the 3 channels of one pixel, y is [b][p]).  An OPERATION is what is done to the n entries v of one group and
// its measurement: OpA, OpApinv, OpProject, OpGd<phase>.  group_kernel<Layout, Op> is the one kernel, with_layout the one place
// that picks a layout; 12 layouts x 6 operations = 72 instantiations.
// One thread per group; the sum runs i = 0 .. n-1 as separately rounded products and additions, every update is one fused
// multiply-add.  Bandwidth-bound: no LDS, no MFMA.  Adjacent threads take adjacent blocks of one block-row, so a wavefront's row
// loads are contiguous; with r = 2 / 4 / 8 and a 16-byte aligned tensor a row is one float2 / float4 / two float4.
#include "common.h"
#include "gd.h"
#include <algorithm>

namespace {
constexpr int NT = 256;
static_assert(NT == GD_NT, "the GD helpers reduce over GD_NT threads");

// ---- layouts: groups(d) per sample, and load / store of the N entries of group g of sample blockIdx.y --------------------------
template <int R, bool VEC> struct BlockLayout {                  // x: [B][C][H][W] ; y: [B][C][H/R][W/R]
    static constexpr int N = R * R;
    static __host__ __device__ int64_t groups(const nlc_group_desc& d) { return (int64_t)d.C * (d.H / R) * (d.W / R); }

    float* xb;
    int W, Wb;
    __device__ BlockLayout(float* x, const nlc_group_desc& d) : xb(x + (int64_t)blockIdx.y * d.C * d.H * d.W), W(d.W), Wb(d.W / R) {}

    __device__ __forceinline__ float* corner(int64_t g) const {
        if constexpr (R == 1) return xb + g;                     // the blocks are the entries: no division left to the optimiser
        const int64_t row = g / Wb;                              // c * (H/R) + by: the block-row, counted over all channels
        const int bx = (int)(g - row * Wb);
        return xb + row * R * W + (int64_t)bx * R;
    }
    __device__ __forceinline__ void load(int64_t g, float* v) const {
        const float* base = corner(g);
#pragma unroll
        for (int j = 0; j < R; ++j) load_row(base + (int64_t)j * W, v + j * R);
    }
    __device__ __forceinline__ void store(int64_t g, const float* v) const {
        float* base = corner(g);
#pragma unroll
        for (int j = 0; j < R; ++j) store_row(base + (int64_t)j * W, v + j * R);
    }

    static __device__ __forceinline__ void load_row(const float* p, float* v) {
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
    static __device__ __forceinline__ void store_row(float* p, const float* v) {
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
};

struct ChannelLayout {                                           // x: [B][3][HW] ; y: [B][HW]
    static constexpr int N = 3;
    static __host__ __device__ int64_t groups(const nlc_group_desc& d) { return (int64_t)d.H * d.W; }

    float* xb;
    int64_t HW;
    __device__ ChannelLayout(float* x, const nlc_group_desc& d) : xb(x + (int64_t)blockIdx.y * 3 * groups(d)), HW(groups(d)) {}

    __device__ __forceinline__ void load(int64_t g, float* v) const {
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] = xb[c * HW + g];
    }
    __device__ __forceinline__ void store(int64_t g, const float* v) const {
#pragma unroll
        for (int c = 0; c < 3; ++c) xb[c * HW + g] = v[c];
    }
};

// ---- operations: op.apply<N>(v, yg, d, q, acc) on the N entries v of one group and its measurement yg.  Each says whether it
//      reads x (v is loaded first), writes x (v is stored after) and writes y (yg is its result, not its input); `phase` is the
//      gd_pass phase the groups are walked in, PLAIN for a grid-stride loop and nothing else; q / acc are that pass's. ------------
constexpr int PLAIN = -1;
// sum_i w_i v_i, i ascending: n products and n-1 additions, each rounded once (no contraction)
template <int N> __device__ __forceinline__ float group_sum(const float* w, const float* v) {
    float s = __fmul_rn(w[0], v[0]);
#pragma unroll
    for (int i = 1; i < N; ++i) s = __fadd_rn(s, __fmul_rn(w[i], v[i]));
    return s;
}

struct OpA {
    static constexpr bool reads_x = true, writes_x = false, writes_y = true;
    static constexpr int phase = PLAIN;
    template <int N> __device__ __forceinline__ void apply(float* v, float& yg, const nlc_group_desc& d, float, double&) const {
        yg = group_sum<N>(d.w, v);
    }
};

struct OpApinv {
    static constexpr bool reads_x = false, writes_x = true, writes_y = false;
    static constexpr int phase = PLAIN;
    template <int N> __device__ __forceinline__ void apply(float* v, float& yg, const nlc_group_desc& d, float, double&) const {
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = __fmul_rn(d.p[i], yg);
    }
};

struct OpProject {
    static constexpr bool reads_x = true, writes_x = true, writes_y = false;
    static constexpr int phase = PLAIN;
    template <int N> __device__ __forceinline__ void apply(float* v, float& yg, const nlc_group_desc& d, float, double&) const {
        const float r = __fsub_rn(yg, group_sum<N>(d.w, v));
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = __fmaf_rn(d.p[i], r, v[i]);
    }
};

// gradient-descent projection (gd.h): GD_L2_SUM adds r^2 to acc and leaves v alone; GD_L1 / GD_L2_APPLY do
// x_i <- x_i - w_i a,  a = lr m_n (l1) or q r_g (l2), rounded once
template <int PH> struct OpGd {
    static constexpr bool reads_x = true, writes_x = PH != GD_L2_SUM, writes_y = false;
    static constexpr int phase = PH;
    gd_params g;
    template <int N> __device__ __forceinline__ void apply(float* v, float& yg, const nlc_group_desc& d, float q, double& acc) const {
        const float r = __fsub_rn(group_sum<N>(d.w, v), yg);
        if constexpr (PH == GD_L2_SUM) {
            acc += (double)r * (double)r;
        } else {
            const float a = PH == GD_L1 ? __fmul_rn(g.lr, gd_l1_steps(r, g.c, g.n_iter)) : __fmul_rn(q, r);
#pragma unroll
            for (int i = 0; i < N; ++i) v[i] = __fmaf_rn(-d.w[i], a, v[i]);
        }
    }
};

template <class L, class Op> __global__ __launch_bounds__(NT) void group_kernel(float* x, float* y, const nlc_group_desc d, const Op op) {
    const L lay(x, d);
    const int64_t G = L::groups(d);
    float* yb = y + (int64_t)blockIdx.y * G;
    auto group = [&](int64_t g, float q, double& acc) __attribute__((always_inline)) {
        float v[L::N];
        float yg = 0.f;
        if constexpr (Op::reads_x) lay.load(g, v);
        if constexpr (!Op::writes_y) yg = yb[g];
        op.template apply<L::N>(v, yg, d, q, acc);
        if constexpr (Op::writes_y) yb[g] = yg;
        if constexpr (Op::writes_x) lay.store(g, v);
    };
    if constexpr (Op::phase == PLAIN) {
        double unused = 0.0;
        for (int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x; g < G; g += (int64_t)gridDim.x * NT) group(g, 0.f, unused);
    } else {
        gd_pass<Op::phase>(G, op.g, group);
    }
}

// (mode, r, alignment of x) -> layout: f(std::type_identity<Layout>).  A row of R floats starts at a multiple of R floats from
// the tensor's base (W % R == 0), so with R = 2 / 4 / 8 it is aligned for a vector access iff the base is, to 8 / 16 / 16 bytes.
template <class F> void with_layout(const nlc_group_desc& d, const float* x, F f) {
    if (d.mode == NLC_GROUP_CHANNEL) return f(std::type_identity<ChannelLayout>{});
    auto block = [&](auto r) {
        constexpr int R = r();
        constexpr bool kCanVec = R == 2 || R == 4 || R == 8;
        if (kCanVec && ((uintptr_t)x % (R == 2 ? 8 : 16)) == 0) f(std::type_identity<BlockLayout<R, kCanVec>>{});
        else f(std::type_identity<BlockLayout<R, false>>{});
    };
    switch (d.r) {
        case 1: block(std::integral_constant<int, 1>{}); break;
        case 2: block(std::integral_constant<int, 2>{}); break;
        case 3: block(std::integral_constant<int, 3>{}); break;
        case 4: block(std::integral_constant<int, 4>{}); break;
        case 5: block(std::integral_constant<int, 5>{}); break;
        case 6: block(std::integral_constant<int, 6>{}); break;
        case 7: block(std::integral_constant<int, 7>{}); break;
        default: block(std::integral_constant<int, 8>{}); break;
    }
}

// a checked descriptor; the workgroups per sample are gd_grid for a GD phase (the partials, nlc_gd_workspace_bytes) and at most
// 1024 otherwise
template <class Op> void launch_group(float* x, float* y, const nlc_group_desc& d, const Op& op, void* stream) {
    with_layout(d, x, [&](auto layout) {
        using L = typename decltype(layout)::type;
        const int g = Op::phase == PLAIN ? std::min(cdiv(L::groups(d), NT), 1024) : gd_grid(L::groups(d));
        hipLaunchKernelGGL((group_kernel<L, Op>), dim3(g, d.B), dim3(NT), 0, (hipStream_t)stream, x, y, d, op);
    });
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

template <class Op> int run_group(float* x, float* y, const nlc_group_desc& d, void* stream, const char* name) {
    NLC_REQUIRE(x && y, "%s: null pointer", name);
    NLC_TRY(check_group_desc(d, name));
    launch_group(x, y, d, Op{}, stream);
    NLC_CHECK_LAUNCH(name);
    return NLC_OK;
}
}  // namespace

extern "C" int nlc_group_A(const float* x, nlc_group_desc desc, float* y_out, void* stream) {
    return run_group<OpA>(const_cast<float*>(x), y_out, desc, stream, "nlc_group_A");
}

extern "C" int nlc_group_Apinv(const float* y, nlc_group_desc desc, float* x_out, void* stream) {
    return run_group<OpApinv>(x_out, const_cast<float*>(y), desc, stream, "nlc_group_Apinv");
}

extern "C" int nlc_group_project(float* x0, const float* y, nlc_group_desc desc, void* stream) {
    return run_group<OpProject>(x0, const_cast<float*>(y), desc, stream, "nlc_group_project");
}

extern "C" int64_t nlc_gd_workspace_bytes(int B, int64_t entries_per_sample) {
    if (B <= 0 || entries_per_sample <= 0) return 0;
    return (int64_t)B * gd_grid(entries_per_sample) * (int64_t)sizeof(double);
}

extern "C" int nlc_group_gd(float* x0, const float* y, nlc_group_desc desc, float lr, int n_iter, int loss, void* workspace,
                            void* stream) {
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
    return gd_run(name, loss, [&](auto ph) { launch_group(x0, const_cast<float*>(y), desc, OpGd<ph()>{g}, stream); });
}
