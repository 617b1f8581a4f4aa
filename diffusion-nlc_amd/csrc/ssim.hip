// 3-D SSIM of restoration runs: ssim_fn (image_sample.py:571-582) -> calculate_ssim(crop_border=0, test_y_channel=False, ssim3d=True)
// -> _ssim_3d (basicsr/metrics/psnr_ssim.py:157-208,251-337).  Per pair (sample, orig) of [C][H][W] f32 images in [0, 1]:
//   a = round_half_even(sample * 255), b = round_half_even(orig * 255)              (0 .. 255; the product is rounded to f32 first)
//   max_value = max(a) <= 1 ? 1 : 255  (sample only) ;  C1 = (0.01 max_value)^2 ,  C2 = (0.03 max_value)^2
//   E[f] = the 11 x 11 x 11 Gaussian (sigma 1.5, normalised) of f over the volume (H, W, C), replicate padding of 5 on all three axes,
//          for f = a, b, a^2, b^2, ab
//   ssim = mean over H W C of (2 mu1 mu2 + C1)(2 s12 + C2) / ((mu1^2 + mu2^2 + C1)(s1 + s2 + C2)) ,  s1 = E[a^2] - E[a]^2  etc.
// The reference builds a Conv3d per image and runs five dense 1331-tap convolutions.  The weights are g_d g_h g_w, so the operator
// is separable: 11 taps along a row, 11 down a column, and on the channel axis, where replicate padding folds the 11 taps onto the
// C <= 4 channels there are, a C x C matrix  M[c][c'] = sum_j g_j [clamp(c + j - 5, 0, C - 1) == c'].  That differs from the dense
// form in rounding only.
// One workgroup takes a TH x TW tile of one pair, all channels: it loads the tile plus a halo of 5 (replicate = the global index
// is clamped, so no load leaves the image), quantises on load and keeps a and b in LDS; per channel it runs the row pass of the five
// fields into LDS and the column pass into registers; each thread then owns all channels of its two pixels, applies M, evaluates the
// map for BOTH constant pairs and the workgroup writes three doubles: the two map sums and whether any own a exceeds 1.  No filtered
// field goes to global memory.  ssim3d_finalise_kernel adds a pair's tile sums in a fixed order and picks the constant pair.  No
// floating-point atomics: the same input gives the same bits on every run.
// LDS for C = 4: a, b 2 x 4 x 26 x 42 x 4 B = 34,944 B ; row-pass fields 5 x 26 x 32 x 4 B = 16,640 B ; 51.6 KiB, three workgroups per CU.
// Row stride 42 / 32 floats with x on consecutive lanes: every ds_read_b32 / ds_write_b32 of a half-wave hits 32 distinct banks.
#include "common.h"
#include "gd.h"

namespace {
constexpr int NT = GD_NT;                // gd_block_sum reduces over GD_NT threads
constexpr int RAD = 5, TAPS = 11;
constexpr int TH = 16, TW = 32;          // pixels per workgroup; TH * TW = 2 * NT: two pixels per thread, rows ty and ty + 8
constexpr int HH = TH + 2 * RAD, HWD = TW + 2 * RAD;
constexpr int PARTS = 3;                 // doubles per tile: map sum with max_value = 1, with 255, count of own a > 1
static_assert(TH * TW == 2 * NT && TW == 32, "the pixel-to-thread map below");

struct ssim_tables {
    float g[TAPS];                       // the normalised Gaussian, rounded once
    float m[16];                         // M[c][c'] at m[c * 4 + c'], summed in double, rounded once
    float c1[2], c2[2];                  // [0]: max_value = 1, [1]: 255
};

// torch.round(x * 255).to(torch.uint8) for x in [0, 1]; anything else is clamped into 0 .. 255
__device__ __forceinline__ float quantise(float x) { return fminf(fmaxf(rintf(__fmul_rn(x, 255.f)), 0.f), 255.f); }

__device__ __forceinline__ float ssim_value(float mu1, float mu2, float e11, float e22, float e12, float c1, float c2) {
    const float m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
    const float s1 = e11 - m11, s2 = e22 - m22, s12 = e12 - m12;
    return ((2.f * m12 + c1) * (2.f * s12 + c2)) / ((m11 + m22 + c1) * (s1 + s2 + c2));
}

// grid: (tiles in x, tiles in y, min(N, 65535)) ; parts: [N][tiles][PARTS]
template <int C>
__global__ __launch_bounds__(NT) void ssim3d_map_kernel(const float* __restrict__ sample, const float* __restrict__ orig, int N, int P,
                                                        int H, int W, const ssim_tables t, double* __restrict__ parts) {
    __shared__ float sA[C][HH][HWD];
    __shared__ float sB[C][HH][HWD];
    __shared__ float sF[5][HH][TW];
    __shared__ double sh[NT / 64];
    const int tid = threadIdx.x;
    const int x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
    const int64_t tiles = (int64_t)gridDim.x * gridDim.y;
    const int64_t tile = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const int64_t HW = (int64_t)H * W;
    const int tx = tid & (TW - 1), ty = tid / TW;                // own pixels: (ty, tx) and (ty + 8, tx) of the tile

    for (int n = blockIdx.z; n < N; n += gridDim.z) {
        const float* sa = sample + (int64_t)n * C * HW;
        const float* so = orig + (int64_t)(n % P) * C * HW;
        __syncthreads();                                         // the previous pair's reads of sA / sB are done
        for (int i = tid; i < C * HH * HWD; i += NT) {
            const int c = i / (HH * HWD), r = i - c * (HH * HWD);
            const int y = r / HWD, x = r - y * HWD;
            const int gy = min(max(y0 + y - RAD, 0), H - 1), gx = min(max(x0 + x - RAD, 0), W - 1);
            const int64_t src = (int64_t)c * HW + (int64_t)gy * W + gx;
            sA[c][y][x] = quantise(sa[src]);
            sB[c][y][x] = quantise(so[src]);
        }
        float v[2][5][C];                                        // [own pixel][field][channel] after the row and column passes
#pragma unroll
        for (int c = 0; c < C; ++c) {
            __syncthreads();                                     // sA / sB are loaded (c = 0) ; the column pass of c - 1 has read sF
            for (int i = tid; i < HH * TW; i += NT) {
                const int y = i / TW, x = i - y * TW;
                float h[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < TAPS; ++j) {
                    const float a = sA[c][y][x + j], b = sB[c][y][x + j], g = t.g[j];
                    h[0] = fmaf(g, a, h[0]);
                    h[1] = fmaf(g, b, h[1]);
                    h[2] = fmaf(g, a * a, h[2]);                 // a, b are integers <= 255: the products are exact
                    h[3] = fmaf(g, b * b, h[3]);
                    h[4] = fmaf(g, a * b, h[4]);
                }
#pragma unroll
                for (int f = 0; f < 5; ++f) sF[f][y][x] = h[f];
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 2; ++q)
#pragma unroll
                for (int f = 0; f < 5; ++f) {
                    float s = 0.f;
#pragma unroll
                    for (int j = 0; j < TAPS; ++j) s = fmaf(t.g[j], sF[f][ty + 8 * q + j][tx], s);
                    v[q][f][c] = s;
                }
        }
        double acc1 = 0.0, acc255 = 0.0, bright = 0.0;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int py = ty + 8 * q;
            if (y0 + py >= H || x0 + tx >= W) continue;          // outside the image: this pixel belongs to no one
#pragma unroll
            for (int c = 0; c < C; ++c) {
                float u[5];
#pragma unroll
                for (int f = 0; f < 5; ++f) {
                    float s = 0.f;
#pragma unroll
                    for (int k = 0; k < C; ++k) s = fmaf(t.m[c * 4 + k], v[q][f][k], s);
                    u[f] = s;
                }
                acc1 += (double)ssim_value(u[0], u[1], u[2], u[3], u[4], t.c1[0], t.c2[0]);
                acc255 += (double)ssim_value(u[0], u[1], u[2], u[3], u[4], t.c1[1], t.c2[1]);
                if (sA[c][py + RAD][tx + RAD] > 1.f) bright += 1.0;
            }
        }
        acc1 = gd_block_sum(acc1, sh);
        acc255 = gd_block_sum(acc255, sh);
        bright = gd_block_sum(bright, sh);
        if (tid == 0) {
            double* p = parts + ((int64_t)n * tiles + tile) * PARTS;
            p[0] = acc1; p[1] = acc255; p[2] = bright;
        }
    }
}

// grid: min(N, 65535) ; out[n] = (sum over the pair's tiles, tile index ascending per thread, then gd_block_sum) / (H W C)
__global__ __launch_bounds__(NT) void ssim3d_finalise_kernel(const double* __restrict__ parts, int N, int64_t tiles, double count,
                                                             double* __restrict__ out) {
    __shared__ double sh[NT / 64];
    for (int n = blockIdx.x; n < N; n += gridDim.x) {
        const double* p = parts + (int64_t)n * tiles * PARTS;
        double s1 = 0.0, s255 = 0.0, bright = 0.0;
        for (int64_t i = threadIdx.x; i < tiles; i += NT) {
            s1 += p[i * PARTS];
            s255 += p[i * PARTS + 1];
            bright += p[i * PARTS + 2];
        }
        s1 = gd_block_sum(s1, sh);
        s255 = gd_block_sum(s255, sh);
        bright = gd_block_sum(bright, sh);
        if (threadIdx.x == 0) out[n] = (bright > 0.0 ? s255 : s1) / count;
    }
}

ssim_tables make_tables(int C) {
    ssim_tables t{};
    double g[TAPS], sum = 0.0;
    for (int i = 0; i < TAPS; ++i) { g[i] = std::exp(-(double)((i - RAD) * (i - RAD)) / (2.0 * 1.5 * 1.5)); sum += g[i]; }
    for (int i = 0; i < TAPS; ++i) { g[i] /= sum; t.g[i] = (float)g[i]; }
    for (int c = 0; c < C; ++c) {
        double row[4] = {0.0, 0.0, 0.0, 0.0};
        for (int j = 0; j < TAPS; ++j) {
            const int k = c + j - RAD;
            row[k < 0 ? 0 : (k > C - 1 ? C - 1 : k)] += g[j];
        }
        for (int k = 0; k < C; ++k) t.m[c * 4 + k] = (float)row[k];
    }
    const double mv[2] = {1.0, 255.0};
    for (int i = 0; i < 2; ++i) {
        t.c1[i] = (float)((0.01 * mv[i]) * (0.01 * mv[i]));
        t.c2[i] = (float)((0.03 * mv[i]) * (0.03 * mv[i]));
    }
    return t;
}

constexpr int MAX_EDGE = 65536;          // tiles in y <= 4096 (the grid's y limit is 65535) and every index fits the kernels' arithmetic
bool shape_ok(int N, int C, int H, int W) { return N >= 1 && C >= 1 && C <= 4 && H >= 1 && W >= 1 && H <= MAX_EDGE && W <= MAX_EDGE; }
int64_t tiles_of(int H, int W) { return (int64_t)cdiv(H, TH) * cdiv(W, TW); }
}  // namespace

extern "C" int64_t nlc_ssim3d_workspace_bytes(int N, int C, int H, int W) {
    if (!shape_ok(N, C, H, W)) return 0;
    return (int64_t)N * tiles_of(H, W) * PARTS * (int64_t)sizeof(double);
}

extern "C" int nlc_ssim3d(const float* sample, const float* orig, int N, int P, int C, int H, int W, double* out, void* workspace,
                          void* stream) {
    const char* name = "nlc_ssim3d";
    NLC_REQUIRE(sample && orig && out && workspace, "%s: null pointer", name);
    NLC_REQUIRE(N >= 1 && H >= 1 && W >= 1, "%s: bad shape N=%d H=%d W=%d", name, N, H, W);
    NLC_REQUIRE(C >= 1 && C <= 4, "%s: C = %d outside 1..4", name, C);
    NLC_REQUIRE(H <= MAX_EDGE && W <= MAX_EDGE, "%s: H=%d W=%d above %d", name, H, W, MAX_EDGE);
    NLC_REQUIRE(P >= 1 && P <= N && N % P == 0, "%s: P = %d must divide N = %d", name, P, N);
    NLC_REQUIRE(((uintptr_t)workspace % 8) == 0 && ((uintptr_t)out % 8) == 0, "%s: workspace or out is not 8-byte aligned", name);
    NLC_REQUIRE(((uintptr_t)sample % 4) == 0 && ((uintptr_t)orig % 4) == 0, "%s: sample or orig is not 4-byte aligned", name);
    hipStream_t s = (hipStream_t)stream;
    const ssim_tables t = make_tables(C);
    double* parts = (double*)workspace;
    const dim3 grid(cdiv(W, TW), cdiv(H, TH), N < 65535 ? N : 65535);
    switch (C) {
        case 1: hipLaunchKernelGGL((ssim3d_map_kernel<1>), grid, dim3(NT), 0, s, sample, orig, N, P, H, W, t, parts); break;
        case 2: hipLaunchKernelGGL((ssim3d_map_kernel<2>), grid, dim3(NT), 0, s, sample, orig, N, P, H, W, t, parts); break;
        case 3: hipLaunchKernelGGL((ssim3d_map_kernel<3>), grid, dim3(NT), 0, s, sample, orig, N, P, H, W, t, parts); break;
        default: hipLaunchKernelGGL((ssim3d_map_kernel<4>), grid, dim3(NT), 0, s, sample, orig, N, P, H, W, t, parts); break;
    }
    NLC_CHECK_LAUNCH(name);
    hipLaunchKernelGGL(ssim3d_finalise_kernel, dim3(N < 65535 ? N : 65535), dim3(NT), 0, s, parts, N, tiles_of(H, W),
                       (double)H * (double)W * (double)C, out);
    NLC_CHECK_LAUNCH(name);
    return NLC_OK;
}
