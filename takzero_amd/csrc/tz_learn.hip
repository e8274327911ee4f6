// tz_learn.hip — the `learn` training step on MI355X: forward in training mode, the
// three losses, backward and Adam (learn/src/main.rs:376-423; graph net5.rs:44-191, residual.rs:13-63).
//
// The reference trains in fp32 through LibTorch; so does this: every contraction is an fp32 MFMA GEMM
// (v_mfma_f32_32x32x2_f32) whose A operand is the im2col view of an NHWC tensor, gathered by the tile loader
// (no col matrix exists) — at the reference's batch of 128 positions a step is 0.46 TFLOP:
//
//   activations   NHWC fp32  [M = batch*n*n][256]            (everything of one step stays resident)
//   conv weights  GEMM layout [K = 9*cin (padded to 64)][cout (padded to 64)], k = tap*cin + ci
//   forward       c = im2col(x) x W;  BatchNorm with batch statistics;  ReLU (+ skip)
//   backward      dW = im2col(x)^T x dc  (A-transposed GEMM);  dx = im2col(dc) x W'  with W' = taps mirrored, ci/co swapped
//   parameters, gradients and the two Adam moments live in four parallel arenas; one Adam launch per step.
//
// Optional (tz_trainer_rnd_enable, off by default): net5's RND predictor is trained in the same step (net5.rs:193-218;
// learn/src/main.rs:404-405) by a chain of small launches on a stream of its own, see "RND distillation" below.  net4_rnd's predictor
// tower has the same switch (tz_trainer_rnd4_enable); its kernels are a unit of their own, tz_learn_rnd4.hip.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>

#include <map>
#include <string>
#include <vector>

#include "tz_learn_rnd4.h"
#include "tz_nn.h"

namespace {

constexpr int FILTERS = 256;
constexpr float BN_EPS = 1e-5f;       // tch BatchNormConfig::default
constexpr float BN_MOMENTUM = 0.1f;   // tch BatchNormConfig::default
constexpr int SPLITS = 64;            // row splits of the per-channel reductions (8 x 64 workgroups)
constexpr float MINIMUM_UBE_TARGET = -10.0f;  // learn/src/main.rs:47
constexpr float MAXIMUM_VARIANCE = 4.0f;      // net5.rs:23

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------------------------------------
// C[M][N] = (accumulate ? C : 0) + A x B (+ bias[n]).  M, N multiples of 64, K multiple of 32.
// AT = false: A(m,k) = A[m*lda + k];  AT = true: A(m,k) = A[k*lda + m].   B(k,n) = B[k*ldb + n].
// One 64x64 tile per workgroup of 8 waves = two groups of 4: group g multiplies the k-slabs 2i+g (16 deep), each
// of its waves owning a 32x32 quadrant, so every SIMD has two waves to interleave; the two partial tiles are added
// through LDS at the end (fixed order: deterministic).  Slabs are double buffered in LDS (one barrier per step) and
// the next pair is fetched into registers while the MFMAs of the current one run.
//
// GATHER: A is not a stored matrix but the im2col view of an NHWC tensor x [pixels][gc]: A(pixel, tap*gc + c) =
// x[(board, y + tap/3 - 1, x + tap%3 - 1)][c], zero off the board and for k >= 9*gc (the K padding).  The loader
// computes that address itself (4 consecutive channels per thread), so no col matrix is ever written or read.
template <bool AT, bool GATHER>
__global__ __launch_bounds__(512) void gemm_f32_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                       float* __restrict__ C, const float* __restrict__ bias, int K,
                                                       int lda, int ldb, int ldc, int accumulate, int gn, int gc) {
    __shared__ float As[2][2][16][68];  // [buffer][group][k][m]
    __shared__ float Bs[2][2][16][68];
    const int g = threadIdx.x >> 8, t = threadIdx.x & 255, lane = t & 63, wave = t >> 6;
    const size_t m0 = (size_t)blockIdx.x * 64, n0 = (size_t)blockIdx.y * 64;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    const int ak = AT ? (t >> 4) : (t & 3) * 4, am = AT ? (t & 15) * 4 : (t >> 2);
    const int bk = t >> 4, bn = (t & 15) * 4;
    const float* ap = AT ? A + (size_t)(16 * g + ak) * lda + m0 + am : A + (m0 + am) * lda + 16 * g + ak;
    const float* bp = B + (size_t)(16 * g + bk) * ldb + n0 + bn;
    const size_t astep = AT ? (size_t)32 * lda : 32, bstep = (size_t)32 * ldb;
    // gather state.  The address arithmetic of the im2col view is taken out of the loop (integer VALU work inside an MFMA
    // loop is expensive: it competes with the other wave of the SIMD for issue slots): a small LDS table holds, for every
    // (tap, pixel of a board), the offset of the source pixel or -1 off the board; per step a thread advances one counter,
    // reads one table entry and adds.
    //   !AT: the thread's pixel is fixed (row m0+am), its k = tap*gc + c advances by 32 per step.
    //   AT : its 4 k-indices are fixed (m0+am..+3 = one tap, 4 channels), its pixel advances by 32 per step.
    __shared__ int srcoff[9][40];   // [tap][pixel in board] -> (source pixel in board) * gc, or -1
    const int gnn = gn * gn;
    int g_b = 0, g_lp = 0, g_tap = 0, g_c = 0;          // board, pixel inside the board, tap, channel
    if (GATHER) {
        for (int i = threadIdx.x; i < 9 * gnn; i += 512) {
            const int tap = i / gnn, lp = i - tap * gnn, y = lp / gn + tap / 3 - 1, x = lp % gn + tap % 3 - 1;
            srcoff[tap][lp] = (y >= 0 && y < gn && x >= 0 && x < gn) ? (y * gn + x) * gc : -1;
        }
        const int pix = AT ? 16 * g + ak : (int)m0 + am, k = AT ? (int)m0 + am : 16 * g + ak;
        g_b = pix / gnn;
        g_lp = pix - g_b * gnn;
        g_tap = k / gc;            // >= 9 marks the K padding
        g_c = k - g_tap * gc;
        __syncthreads();
    }
    const float* g_row = A + (size_t)g_b * gnn * gc;    // start of the thread's current board
    auto gather = [&]() -> float4 {
        const int off = g_tap < 9 ? srcoff[g_tap][g_lp] : -1;
        if (off < 0) return make_float4(0.f, 0.f, 0.f, 0.f);
        return *(const float4*)(g_row + off + g_c);
    };
    auto gather_advance = [&]() {
        if (AT) {
            g_lp += 32;
            while (g_lp >= gnn) {
                g_lp -= gnn;
                g_row += gnn * gc;
            }
        } else {
            g_c += 32;
            while (g_c >= gc) {
                g_c -= gc;
                g_tap++;
            }
        }
    };
    f32x16 acc;
#pragma unroll
    for (int i = 0; i < 16; i++) acc[i] = 0.f;
    // operands of k-steps i and i + 1 are in flight while step i - 1 multiplies: one step (a thousand cycles) does not cover a
    // miss of the XCD's L2 on the gathered view, two do
    float4 ra0, ra1, rb0, rb1;   // named, not an array: a slot picked at run time would send them to scratch
    auto fetch = [&](float4& ra, float4& rb) {
        ra = GATHER ? gather() : *(const float4*)ap;
        rb = *(const float4*)bp;
    };
    auto advance = [&]() {
        bp += bstep;
        if (GATHER) gather_advance();
        else ap += astep;
    };
    fetch(ra0, rb0);
    if (32 < K) {
        advance();
        fetch(ra1, rb1);
    }
    auto step = [&](int k0, int buf, float4& ra, float4& rb) {
        if (AT) {
            *(float4*)&As[buf][g][ak][am] = ra;
        } else {
            As[buf][g][ak + 0][am] = ra.x;
            As[buf][g][ak + 1][am] = ra.y;
            As[buf][g][ak + 2][am] = ra.z;
            As[buf][g][ak + 3][am] = ra.w;
        }
        *(float4*)&Bs[buf][g][bk][bn] = rb;
        __syncthreads();
        if (k0 + 64 < K) {
            advance();
            fetch(ra, rb);
        }
#pragma unroll
        for (int kk = 0; kk < 16; kk += 2) {
            const float a = As[buf][g][kk + (lane >> 5)][wm + (lane & 31)];
            const float b = Bs[buf][g][kk + (lane >> 5)][wn + (lane & 31)];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
    };
    for (int k0 = 0; k0 < K; k0 += 64) {
        step(k0, 0, ra0, rb0);
        if (k0 + 32 < K) step(k0 + 32, 1, ra1, rb1);
    }
    __syncthreads();
    float* red = &As[0][0][0][0];  // 64 x 64 partial tile of group 1
    if (g == 1) {
#pragma unroll
        for (int r = 0; r < 16; r++) red[(wm + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3)) * 64 + wn + (lane & 31)] = acc[r];
    }
    __syncthreads();
    if (g == 1) return;
    const size_t n = n0 + wn + (lane & 31);
    const float bv = bias ? bias[n] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; r++) {
        const int ml = wm + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
        const size_t m = m0 + ml;
        float v = acc[r] + red[ml * 64 + wn + (lane & 31)] + bv;
        if (accumulate) v += C[m * ldc + n];
        C[m * ldc + n] = v;
    }
}

// ------------------------------------------------------------------------------------------------
// The same product, its work cut so that every CU gets an equal share ("stream-K").  At the reference's batch of 128 a forward or
// data-gradient GEMM is 200 tiles of 64x64 and a weight-gradient GEMM 144 — for 256 CUs.  Here the (tile, k-slab) pairs are laid
// out in one line, tile by tile, and workgroup w of G takes the contiguous range [w T / G, (w + 1) T / G): it walks through at most
// one partial tile, whole tiles, one partial tile.  A whole tile gets the usual epilogue; a partial one goes to the workgroup's
// slot in a workspace, and gemm_fixup_kernel adds a tile's parts in ascending k (ascending workgroup) — a fixed order, so the
// result does not depend on timing.  A workgroup is 4 waves, one 32x32 quadrant each over the full slab depth of 32: two of them
// share a CU (G = 2 x CUs), each with its own barriers, so one's barrier wait is the other's MFMA time.
struct SkRange {
    long long begin, end;
};
__device__ __host__ inline SkRange sk_range(int w, int G, long long total) {
    return SkRange{(long long)w * total / G, (long long)(w + 1) * total / G};
}

template <bool AT, bool GATHER>
__global__ __launch_bounds__(256) void gemm_sk_kernel(const float* __restrict__ A, const float* __restrict__ B, float* __restrict__ C,
                                                      const float* __restrict__ bias, int K, int lda, int ldb, int ldc, int accumulate,
                                                      int gn, int gc, int tiles_m, long long total, float* __restrict__ ws) {
    __shared__ float As[2][32][68];  // [buffer][k][m]
    __shared__ float Bs[2][32][68];
    __shared__ int srcoff[9][40];    // [tap][pixel in board] -> (source pixel in board) * gc, or -1 (see gemm_f32_kernel)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
    const int S = K / 32, gnn = gn * gn;
    const SkRange mine = sk_range(blockIdx.x, gridDim.x, total);
    if (GATHER) {
        for (int i = t; i < 9 * gnn; i += 256) {
            const int tap = i / gnn, lp = i - tap * gnn, y = lp / gn + tap / 3 - 1, x = lp % gn + tap % 3 - 1;
            srcoff[tap][lp] = (y >= 0 && y < gn && x >= 0 && x < gn) ? (y * gn + x) * gc : -1;
        }
        __syncthreads();
    }
    // loader: two float4 per thread and operand per slab.  !AT: 4 consecutive k of rows am, am + 32;  AT: 4 consecutive m of k-rows ak, ak + 16
    const int ak = AT ? (t >> 4) : (t & 7) * 4, am = AT ? (t & 15) * 4 : (t >> 3);
    const int bk = t >> 4, bn = (t & 15) * 4;
    for (long long cur = mine.begin; cur < mine.end;) {
        const int tile = (int)(cur / S), ks0 = (int)(cur - (long long)tile * S);
        const int ks1 = (int)((long long)S < ks0 + (mine.end - cur) ? (long long)S : ks0 + (mine.end - cur));
        const size_t m0 = (size_t)(tile % tiles_m) * 64, n0 = (size_t)(tile / tiles_m) * 64;
        // state of the thread's two fetches per slab (h = 0, 1): plain pointer, or board / pixel inside the board / tap / channel of the
        // gathered view.  Named objects throughout: an array indexed by h would live in scratch.
        struct Src {
            const float* ap;
            const float* row;
            int lp, tap, c;
        };
        auto src_init = [&](int h) -> Src {
            Src q{A, A, 0, 0, 0};
            if (GATHER) {
                const int pix = AT ? 32 * ks0 + ak + 16 * h : (int)m0 + am + 32 * h, k = AT ? (int)m0 + am : 32 * ks0 + ak;
                const int b = pix / gnn;
                q.lp = pix - b * gnn;
                q.row = A + (size_t)b * gnn * gc;
                q.tap = k / gc;            // >= 9 marks the K padding
                q.c = k - q.tap * gc;
            } else {
                q.ap = AT ? A + (size_t)(32 * ks0 + ak + 16 * h) * lda + m0 + am : A + (m0 + am + 32 * h) * lda + 32 * ks0 + ak;
            }
            return q;
        };
        Src s0 = src_init(0), s1 = src_init(1);
        const float* bp = B + (size_t)(32 * ks0 + bk) * ldb + n0 + bn;
        const size_t astep = AT ? (size_t)32 * lda : 32, bstep = (size_t)32 * ldb, bhalf = (size_t)16 * ldb;
        auto load_a = [&](const Src& q) -> float4 {
            if (GATHER) {
                const int off = q.tap < 9 ? srcoff[q.tap][q.lp] : -1;
                return off < 0 ? make_float4(0.f, 0.f, 0.f, 0.f) : *(const float4*)(q.row + off + q.c);
            }
            return *(const float4*)q.ap;
        };
        auto advance_a = [&](Src& q) {
            if (!GATHER) {
                q.ap += astep;
            } else if (AT) {
                q.lp += 32;
                while (q.lp >= gnn) {
                    q.lp -= gnn;
                    q.row += gnn * gc;
                }
            } else {
                q.c += 32;
                while (q.c >= gc) {
                    q.c -= gc;
                    q.tap++;
                }
            }
        };
        struct Slab {
            float4 a0, a1, b0, b1;
        };
        auto fetch = [&](Slab& f) {
            f.a0 = load_a(s0);
            f.a1 = load_a(s1);
            f.b0 = *(const float4*)bp;
            f.b1 = *(const float4*)(bp + bhalf);
        };
        auto advance = [&]() {
            bp += bstep;
            advance_a(s0);
            advance_a(s1);
        };
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; i++) acc[i] = 0.f;
        Slab f0, f1;   // slabs i and i + 1 in flight while slab i - 1 multiplies
        fetch(f0);
        if (ks0 + 1 < ks1) {
            advance();
            fetch(f1);
        }
        auto store_a = [&](int buf, int h, const float4& v) {
            if (AT) {
                *(float4*)&As[buf][ak + 16 * h][am] = v;
            } else {
                As[buf][ak + 0][am + 32 * h] = v.x;
                As[buf][ak + 1][am + 32 * h] = v.y;
                As[buf][ak + 2][am + 32 * h] = v.z;
                As[buf][ak + 3][am + 32 * h] = v.w;
            }
        };
        auto step = [&](int ks, int buf, Slab& f) {
            store_a(buf, 0, f.a0);
            store_a(buf, 1, f.a1);
            *(float4*)&Bs[buf][bk][bn] = f.b0;
            *(float4*)&Bs[buf][bk + 16][bn] = f.b1;
            __syncthreads();
            if (ks + 2 < ks1) {
                advance();
                fetch(f);
            }
#pragma unroll
            for (int kk = 0; kk < 32; kk += 2) {
                const float a = As[buf][kk + (lane >> 5)][wm + (lane & 31)];
                const float b = Bs[buf][kk + (lane >> 5)][wn + (lane & 31)];
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
            }
        };
        for (int ks = ks0; ks < ks1; ks += 2) {
            step(ks, 0, f0);
            if (ks + 1 < ks1) step(ks + 1, 1, f1);
        }
        __syncthreads();   // the next segment's first store goes to buffer 0
        const bool whole = ks0 == 0 && ks1 == S;
        if (whole) {
            const size_t n = n0 + wn + (lane & 31);
            const float bv = bias ? bias[n] : 0.f;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const size_t m = m0 + wm + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3);
                float v = acc[r] + bv;
                if (accumulate) v += C[m * ldc + n];
                C[m * ldc + n] = v;
            }
        } else {   // slot 0: the range's first segment, slot 1: its last
            float* part = ws + ((size_t)blockIdx.x * 2 + (cur == mine.begin ? 0 : 1)) * 4096;
#pragma unroll
            for (int r = 0; r < 16; r++) part[(wm + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3)) * 64 + wn + (lane & 31)] = acc[r];
        }
        cur += ks1 - ks0;
    }
}

// One workgroup per tile: nothing to do for a tile that one workgroup multiplied whole; otherwise the parts, in ascending k.
// (32-bit range arithmetic: w * total < 2^32 for every launch — 64-bit divisions would be most of this kernel's time.)
__device__ inline unsigned sk_begin32(unsigned w, unsigned G, unsigned total) { return w * total / G; }

__global__ __launch_bounds__(256) void gemm_fixup_kernel(float* __restrict__ C, const float* __restrict__ bias, int S, int ldc, int accumulate,
                                                         int tiles_m, unsigned total, unsigned G, const float* __restrict__ ws) {
    const unsigned tile = blockIdx.x;
    const unsigned t0 = tile * (unsigned)S, t1 = t0 + (unsigned)S;
    unsigned w = t0 * G / total;
    while (w > 0 && sk_begin32(w, G, total) > t0) w--;
    while (sk_begin32(w + 1, G, total) <= t0) w++;
    if (sk_begin32(w, G, total) <= t0 && sk_begin32(w + 1, G, total) >= t1) return;
    const size_t m0 = (size_t)(tile % tiles_m) * 64, n0 = (size_t)(tile / tiles_m) * 64;
    float4 v[4];
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    for (; w < G; w++) {
        const unsigned begin = sk_begin32(w, G, total);
        if (begin >= t1) break;
        // its first segment unless the range began in an earlier tile
        const float4* part = reinterpret_cast<const float4*>(ws + ((size_t)w * 2 + (begin >= t0 ? 0 : 1)) * 4096);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float4 p = part[i * 256 + threadIdx.x];
            v[i].x += p.x;
            v[i].y += p.y;
            v[i].z += p.z;
            v[i].w += p.w;
        }
    }
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int e = (i * 256 + threadIdx.x) * 4;
        const size_t m = m0 + (e >> 6), n = n0 + (e & 63);
        float4 x = v[i];
        if (bias) {
            const float4 bv = *reinterpret_cast<const float4*>(bias + n);
            x.x += bv.x;
            x.y += bv.y;
            x.z += bv.z;
            x.w += bv.w;
        }
        float4* dst = reinterpret_cast<float4*>(C + m * ldc + n);
        if (accumulate) {
            const float4 c = *dst;
            x.x += c.x;
            x.y += c.y;
            x.z += c.z;
            x.w += c.w;
        }
        *dst = x;
    }
}

// W'[(tap'*Co + co)][ci] = W[((8-tap')*Ci + ci)][co]: the weight matrix of the data gradient.  ldw / ldo = row strides.
__global__ void mirror_weights_kernel(const float* __restrict__ W, float* __restrict__ out, int Ci, int Co, int ldw,
                                      int ldo) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)9 * Co * Ci) return;
    const int ci = (int)(idx % Ci), co = (int)((idx / Ci) % Co), tap = (int)(idx / ((size_t)Ci * Co));
    out[((size_t)tap * Co + co) * ldo + ci] = W[((size_t)(8 - tap) * Ci + ci) * ldw + co];
}

// per-channel partial sums over a slice of the rows, in double.
// mode 0 (statistics): (x, x*x) of c.   mode 1 (BatchNorm backward): (dy, dy*xhat), dy = da * (a > 0).
__global__ __launch_bounds__(256) void column_partials_kernel(int mode, const float* __restrict__ c,
                                                              const float* __restrict__ da, const float* __restrict__ a,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ invstd, int M,
                                                              double* __restrict__ partial) {
    __shared__ double s1[8][32], s2[8][32];
    const int ch = blockIdx.x * 32 + (threadIdx.x & 31), r = threadIdx.x >> 5;
    const int rows = (M + SPLITS - 1) / SPLITS, lo = blockIdx.y * rows, hi = min(M, lo + rows);
    double x1 = 0.0, x2 = 0.0;
    if (mode == 0) {
        for (int m = lo + r; m < hi; m += 8) {
            const double v = c[(size_t)m * FILTERS + ch];
            x1 += v;
            x2 += v * v;
        }
    } else {
        const float mu = mean[ch], is = invstd[ch];
        for (int m = lo + r; m < hi; m += 8) {
            const size_t i = (size_t)m * FILTERS + ch;
            const float dy = a[i] > 0.f ? da[i] : 0.f;
            x1 += dy;
            x2 += (double)dy * (double)((c[i] - mu) * is);
        }
    }
    s1[r][threadIdx.x & 31] = x1;
    s2[r][threadIdx.x & 31] = x2;
    __syncthreads();
    if (r == 0) {
        for (int i = 1; i < 8; i++) {
            x1 += s1[i][threadIdx.x];
            x2 += s2[i][threadIdx.x];
        }
        partial[((size_t)blockIdx.y * FILTERS + ch) * 2 + 0] = x1;
        partial[((size_t)blockIdx.y * FILTERS + ch) * 2 + 1] = x2;
    }
}

// batch statistics + running statistics (torch: biased variance normalises, unbiased one is tracked)
__global__ void bn_stats_finish_kernel(const double* __restrict__ partial, int M, float* mean, float* invstd,
                                       float* running_mean, float* running_var) {
    const int ch = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int s = 0; s < SPLITS; s++) {
        s1 += partial[((size_t)s * FILTERS + ch) * 2];
        s2 += partial[((size_t)s * FILTERS + ch) * 2 + 1];
    }
    const double mu = s1 / M;
    double var = s2 / M - mu * mu;
    if (var < 0.0) var = 0.0;
    mean[ch] = (float)mu;
    invstd[ch] = (float)(1.0 / sqrt(var + (double)BN_EPS));
    running_mean[ch] = (1.f - BN_MOMENTUM) * running_mean[ch] + BN_MOMENTUM * (float)mu;
    running_var[ch] = (1.f - BN_MOMENTUM) * running_var[ch] + BN_MOMENTUM * (float)(var * M / (M - 1));
}

// a = relu(gamma * (c - mean) * invstd + beta (+ skip))
__global__ void bn_apply_kernel(const float* __restrict__ c, const float* __restrict__ mean,
                                const float* __restrict__ invstd, const float* __restrict__ gamma,
                                const float* __restrict__ beta, const float* __restrict__ skip, float* __restrict__ a,
                                size_t total) {
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= total) return;
    const int ch = (int)(i % FILTERS);
    const float4 x = *(const float4*)(c + i), mu = *(const float4*)(mean + ch), is = *(const float4*)(invstd + ch);
    const float4 g = *(const float4*)(gamma + ch), b = *(const float4*)(beta + ch);
    float4 y;
    y.x = (x.x - mu.x) * is.x * g.x + b.x;
    y.y = (x.y - mu.y) * is.y * g.y + b.y;
    y.z = (x.z - mu.z) * is.z * g.z + b.z;
    y.w = (x.w - mu.w) * is.w * g.w + b.w;
    if (skip) {
        const float4 s = *(const float4*)(skip + i);
        y.x += s.x;
        y.y += s.y;
        y.z += s.z;
        y.w += s.w;
    }
    y.x = fmaxf(y.x, 0.f);
    y.y = fmaxf(y.y, 0.f);
    y.z = fmaxf(y.z, 0.f);
    y.w = fmaxf(y.w, 0.f);
    *(float4*)(a + i) = y;
}

// sums of the backward partials -> d gamma, d beta (into the gradient arena) and the two means the data term needs
__global__ void bn_bwd_finish_kernel(const double* __restrict__ partial, int M, float* dgamma, float* dbeta,
                                     float* mean_dy, float* mean_dyx) {
    const int ch = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int s = 0; s < SPLITS; s++) {
        s1 += partial[((size_t)s * FILTERS + ch) * 2];
        s2 += partial[((size_t)s * FILTERS + ch) * 2 + 1];
    }
    dbeta[ch] = (float)s1;
    dgamma[ch] = (float)s2;
    mean_dy[ch] = (float)(s1 / M);
    mean_dyx[ch] = (float)(s2 / M);
}

// dc = gamma * invstd * (dy - mean(dy) - xhat * mean(dy * xhat)),  dy = da * (a > 0);  dskip (optional) = dy
__global__ void bn_bwd_apply_kernel(const float* __restrict__ c, const float* __restrict__ da,
                                    const float* __restrict__ a, const float* __restrict__ mean,
                                    const float* __restrict__ invstd, const float* __restrict__ gamma,
                                    const float* __restrict__ mean_dy, const float* __restrict__ mean_dyx,
                                    float* __restrict__ dc, float* __restrict__ dskip, size_t total) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int ch = (int)(i % FILTERS);
    const float dy = a[i] > 0.f ? da[i] : 0.f;
    const float xhat = (c[i] - mean[ch]) * invstd[ch];
    dc[i] = gamma[ch] * invstd[ch] * (dy - mean_dy[ch] - xhat * mean_dyx[ch]);
    if (dskip) dskip[i] = dy;
}

// value / UBE heads forward: conv1x1 (256 -> 1) + bias, ReLU, Linear (nn -> 1), tanh for value.  One wave per board.
// hp = [wv 256 | bv | wl nn | bl] (value) and the same for ube; pre[2][M] keeps the conv outputs for backward.
__global__ __launch_bounds__(64) void heads_fwd_kernel(const float* __restrict__ T, const float* __restrict__ vconv_w,
                                                       const float* __restrict__ vconv_b, const float* __restrict__ vlin_w,
                                                       const float* __restrict__ vlin_b, const float* __restrict__ uconv_w,
                                                       const float* __restrict__ uconv_b, const float* __restrict__ ulin_w,
                                                       const float* __restrict__ ulin_b, int nn, float* pre, int M,
                                                       float* value, float* ube) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float pv = 0.f, pu = 0.f;
    if (lane < nn) {
        const float* row = T + ((size_t)b * nn + lane) * FILTERS;
        float sv = 0.f, su = 0.f;
        for (int c = 0; c < FILTERS; c++) {
            sv += row[c] * vconv_w[c];
            su += row[c] * uconv_w[c];
        }
        sv += vconv_b[0];
        su += uconv_b[0];
        pre[(size_t)b * nn + lane] = sv;
        pre[(size_t)M + (size_t)b * nn + lane] = su;
        pv = fmaxf(sv, 0.f) * vlin_w[lane];
        pu = fmaxf(su, 0.f) * ulin_w[lane];
    }
    for (int o = 32; o > 0; o >>= 1) {
        pv += __shfl_down(pv, o);
        pu += __shfl_down(pu, o);
    }
    if (lane == 0) {
        value[b] = tanhf(pv + vlin_b[0]);
        ube[b] = pu + ulin_b[0];
    }
}

// heads backward.  Per board partial gradients (summed over boards in board order by heads_reduce_kernel):
// part[b] = [d vconv_w 256 | d vconv_b | d vlin_w nn | d vlin_b | the same for ube], and the value head's
// contribution to dT (the UBE head reads a detached trunk: net5.rs:188-189).
__global__ __launch_bounds__(64) void heads_bwd_kernel(const float* __restrict__ T, const float* __restrict__ vconv_w,
                                                       const float* __restrict__ vlin_w, const float* __restrict__ ulin_w,
                                                       const float* __restrict__ pre, int M, int nn, int batch,
                                                       const float* __restrict__ value, const float* __restrict__ ube,
                                                       const float* __restrict__ tv, const float* __restrict__ tu,
                                                       int train_ube, float* __restrict__ part, int pstride,
                                                       float* __restrict__ dT, float* loss_v, float* loss_u) {
    __shared__ float dv1[64], du1[64];
    const int b = blockIdx.x, lane = threadIdx.x;
    const float v = value[b], u = ube[b];
    const float ev = v - tv[b];
    const float tgt_u = fminf(fmaxf(logf(tu[b]), MINIMUM_UBE_TARGET), logf(MAXIMUM_VARIANCE));  // learn/src/main.rs:360-363
    const float eu = u - tgt_u;
    const float dpre_v = 2.f * ev / batch * (1.f - v * v);
    const float dpre_u = train_ube ? 2.f * eu / batch : 0.f;
    float* P = part + (size_t)b * pstride;
    float* Pu = P + FILTERS + 1 + nn + 1;
    float sv = 0.f, su = 0.f;
    if (lane < nn) {
        const float cv = pre[(size_t)b * nn + lane], cu = pre[(size_t)M + (size_t)b * nn + lane];
        P[FILTERS + 1 + lane] = dpre_v * fmaxf(cv, 0.f);
        Pu[FILTERS + 1 + lane] = dpre_u * fmaxf(cu, 0.f);
        sv = cv > 0.f ? dpre_v * vlin_w[lane] : 0.f;
        su = cu > 0.f ? dpre_u * ulin_w[lane] : 0.f;
    }
    dv1[lane] = sv;
    du1[lane] = su;
    float tsv = sv, tsu = su;
    for (int o = 32; o > 0; o >>= 1) {
        tsv += __shfl_down(tsv, o);
        tsu += __shfl_down(tsu, o);
    }
    if (lane == 0) {
        P[FILTERS] = tsv;
        Pu[FILTERS] = tsu;
        P[FILTERS + 1 + nn] = dpre_v;
        Pu[FILTERS + 1 + nn] = dpre_u;
        loss_v[b] = ev * ev;
        loss_u[b] = train_ube ? eu * eu : 0.f;
    }
    __syncthreads();
    for (int c = lane; c < FILTERS; c += 64) {
        float gv = 0.f, gu = 0.f;
        const float w = vconv_w[c];
        for (int px = 0; px < nn; px++) {
            const size_t i = ((size_t)b * nn + px) * FILTERS + c;
            const float x = T[i];
            gv += dv1[px] * x;
            gu += du1[px] * x;
            dT[i] = dv1[px] * w;
        }
        P[c] = gv;
        Pu[c] = gu;
    }
}

// out[j] = sum over boards (in order) of part[b][j]
__global__ void sum_rows_kernel(const float* __restrict__ part, int rows, int stride, int count, float* __restrict__ out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= count) return;
    float s = 0.f;
    for (int b = 0; b < rows; b++) s += part[(size_t)b * stride + j];
    out[j] = s;
}

// policy loss and its gradient (learn/src/main.rs:384-391): masked_fill(mask, f32::MIN), log_softmax over the
// board's c*nn + px outputs, loss = -sum(logp * target) / batch.  One workgroup per board.
// pol / dpol are [M][np] NHWC (channel c of pixel px); target / mask are [batch][pol_ch * nn] in the reference's order.
__global__ __launch_bounds__(256) void policy_loss_kernel(const float* __restrict__ pol, const float* __restrict__ target,
                                                          const uint8_t* __restrict__ mask, int nn, int pol_ch, int np,
                                                          int batch, float* __restrict__ dpol, float* __restrict__ loss_p) {
    __shared__ float red[256];
    __shared__ float sh_max, sh_sum, sh_tsum;
    const int b = blockIdx.x, t = threadIdx.x, out = pol_ch * nn;
    const float* tg = target + (size_t)b * out;
    const uint8_t* mk = mask + (size_t)b * out;
    float mx = -3.402823466e38f;
    for (int e = t; e < out; e += 256) {
        const int c = e / nn, px = e % nn;
        if (!mk[e]) mx = fmaxf(mx, pol[((size_t)b * nn + px) * np + c]);
    }
    red[t] = mx;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] = fmaxf(red[t], red[t + o]);
        __syncthreads();
    }
    if (t == 0) sh_max = red[0];
    __syncthreads();
    mx = sh_max;
    float se = 0.f, ts = 0.f;
    for (int e = t; e < out; e += 256) {
        const int c = e / nn, px = e % nn;
        if (!mk[e]) se += expf(pol[((size_t)b * nn + px) * np + c] - mx);
        ts += tg[e];
    }
    red[t] = se;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) sh_sum = red[0];
    __syncthreads();
    red[t] = ts;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) sh_tsum = red[0];
    __syncthreads();
    const float lse = mx + logf(sh_sum), tsum = sh_tsum;
    float l = 0.f;
    for (int e = t; e < np * nn; e += 256) {  // every element of the padded tensor gets a gradient (zero in the padding)
        const int c = e / nn, px = e % nn;
        float g = 0.f;
        if (c < pol_ch && !mk[c * nn + px]) {
            const float logp = pol[((size_t)b * nn + px) * np + c] - lse;
            const float tgt = tg[c * nn + px];
            l -= logp * tgt;
            g = (expf(logp) * tsum - tgt) / batch;
        }
        dpol[((size_t)b * nn + px) * np + c] = g;
    }
    red[t] = l;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) loss_p[b] = red[0];
}

// column sums of a [M][ld] matrix (bias gradient of the policy conv): one workgroup per 32 columns, 8 row lanes
__global__ __launch_bounds__(256) void column_sum_kernel(const float* __restrict__ x, int M, int ld, int count,
                                                         float* __restrict__ out) {
    __shared__ double part[8][32];
    const int j = blockIdx.x * 32 + (threadIdx.x & 31), r = threadIdx.x >> 5;
    double s = 0.0;
    if (j < count)
        for (int m = r; m < M; m += 8) s += x[(size_t)m * ld + j];
    part[r][threadIdx.x & 31] = s;
    __syncthreads();
    if (r == 0 && j < count) {
        for (int i = 1; i < 8; i++) s += part[i][threadIdx.x];
        out[j] = (float)s;
    }
}

__global__ void losses_kernel(const float* lp, const float* lv, const float* lu, int batch, float* out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double p = 0.0, v = 0.0, u = 0.0;
    for (int b = 0; b < batch; b++) {
        p += lp[b];
        v += lv[b];
        u += lu[b];
    }
    out[0] = (float)(p / batch);
    out[1] = (float)(v / batch);
    out[2] = (float)(u / batch);
}

// torch.optim.Adam (tch nn::Adam::default(): beta1 0.9, beta2 0.999, eps 1e-8, no weight decay, no amsgrad).
// group[block of 1024 elements]: 0 = not trained, 1 = stepped every call, 2 = the UBE head (stepped when trained),
// 3 = a side arena with a launch of its own, whose step count arrives as t_rnd: the RND predictor, or net4_ensemble's sixteen heads
// (each counts its own steps, as torch's Adam does per parameter).
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ P, const float* __restrict__ G, float* __restrict__ M1,
                                                   float* __restrict__ M2, const uint8_t* __restrict__ group, float lr,
                                                   int t_main, int t_ube, int t_rnd) {
    const int g = group[blockIdx.x];
    const int step = g == 1 ? t_main : g == 2 ? t_ube : g == 3 ? t_rnd : 0;
    if (step <= 0) return;
    const float b1 = 0.9f, b2 = 0.999f, eps = 1e-8f;
    const float bc1 = 1.f - powf(b1, (float)step), bc2 = 1.f - powf(b2, (float)step);
    const float step_size = lr / bc1, bc2_sqrt = sqrtf(bc2);
    const size_t i0 = (size_t)blockIdx.x * 1024 + threadIdx.x * 4;
    for (int j = 0; j < 4; j++) {
        const size_t i = i0 + j;
        const float gr = G[i];
        const float m = b1 * M1[i] + (1.f - b1) * gr;
        const float v = b2 * M2[i] + (1.f - b2) * gr * gr;
        M1[i] = m;
        M2[i] = v;
        P[i] -= step_size * (m / (sqrtf(v) / bc2_sqrt + eps));
    }
}

// ------------------------------------------------------------------------------------------------
// The sixteen heads of net4_ensemble on the step's detached trunk output (eee/src/ensemble.rs:318-351; net4_ensemble.rs:146-171):
// value_i = tanh(Linear_i(relu(conv1x1_i(T) + b_i))), loss_ensemble = mean over [batch][16] of (target - value)^2, gradients of the
// heads' own variables only.  One arena per kind (parameters, gradients, two moments): conv weights [head][256] at ENS_CW, conv
// biases [16] at ENS_CB, linear weights [head][16 squares] at ENS_LW, linear biases [16] at ENS_LB, padded to whole Adam blocks.
constexpr int ENS = TZ_ENSEMBLE_SIZE, ENS_NN = 16, ENS_CW = 0, ENS_CB = ENS * FILTERS, ENS_LW = ENS_CB + ENS, ENS_LB = ENS_LW + ENS * ENS_NN,
              ENS_COUNT = ENS_LB + ENS, ENS_SLOTS = (ENS_COUNT + 1023) / 1024 * 1024;

// forward of one board and what the backward needs of it: thread (square s, head h) takes the conv in channel order, thread h the
// Linear in square order and tanh; then dz = 2 (v - t) / (16 B) * (1 - v^2) (the gradient at the Linear's output), the squared error,
// and per (head, square) the conv output after ReLU and the gradient at the conv's output
__global__ __launch_bounds__(256) void ens_fwd_kernel(const float* __restrict__ T, const float* __restrict__ P, const float* __restrict__ target,
                                                      int batch, float* __restrict__ values, float* __restrict__ relu,
                                                      float* __restrict__ dz, float* __restrict__ dconv, float* __restrict__ err2) {
    __shared__ float pre[ENS][ENS_NN + 1];
    __shared__ float dzs[ENS];
    const int b = blockIdx.x, tid = threadIdx.x, h = tid & 15, s = tid >> 4;
    const float* row = T + ((size_t)b * ENS_NN + s) * FILTERS;
    const float* w = P + ENS_CW + h * FILTERS;
    float acc = 0.f;
    for (int c = 0; c < FILTERS; c++) acc += row[c] * w[c];
    acc += P[ENS_CB + h];
    const float r = fmaxf(acc, 0.f);
    pre[h][s] = r;
    relu[((size_t)b * ENS + h) * ENS_NN + s] = r;
    __syncthreads();
    if (tid < ENS) {
        float lin = 0.f;
        for (int px = 0; px < ENS_NN; px++) lin += pre[tid][px] * P[ENS_LW + tid * ENS_NN + px];
        const float v = tanhf(lin + P[ENS_LB + tid]);
        const float e = v - target[(size_t)b * ENS + tid];
        const float d = 2.f * e / (float)(ENS * batch) * (1.f - v * v);
        values[(size_t)b * ENS + tid] = v;
        err2[(size_t)b * ENS + tid] = e * e;
        dz[(size_t)b * ENS + tid] = d;
        dzs[tid] = d;
    }
    __syncthreads();
    dconv[((size_t)b * ENS + h) * ENS_NN + s] = r > 0.f ? dzs[h] * P[ENS_LW + h * ENS_NN + s] : 0.f;
}

// gradients of head h = blockIdx.x in two stages, every sum in double and in a fixed order.  Stage one, one workgroup per (head, chunk
// of ENS_CHUNK boards): thread c the conv weight's gradient [256] over the chunk's 16 * ENS_CHUNK rows of T (boards in order, squares
// inside a board in order); threads 0..15 the Linear weights', thread 16 the Linear bias's, thread 17 the conv bias's; thread 18 of
// head 0 the chunk's squared errors.  Stage two, one workgroup per head, adds the chunks up in chunk order.
constexpr int ENS_CHUNK = 8, ENS_SMALL = 32;
__global__ __launch_bounds__(256) void ens_bwd_kernel(const float* __restrict__ T, const float* __restrict__ relu, const float* __restrict__ dz,
                                                      const float* __restrict__ dconv, const float* __restrict__ err2,
                                                      double* __restrict__ part, double* __restrict__ small) {
    const int h = blockIdx.x, chunk = blockIdx.y, tid = threadIdx.x, b0 = chunk * ENS_CHUNK;
    double g = 0.0;
    for (int b = b0; b < b0 + ENS_CHUNK; b++)
        for (int s = 0; s < ENS_NN; s++) {
            const float d = dconv[((size_t)b * ENS + h) * ENS_NN + s];
            if (d != 0.f) g += (double)d * (double)T[((size_t)b * ENS_NN + s) * FILTERS + tid];
        }
    part[((size_t)chunk * ENS + h) * FILTERS + tid] = g;
    if (tid >= ENS_SMALL) return;
    double a = 0.0;
    if (tid < ENS_NN) {
        for (int b = b0; b < b0 + ENS_CHUNK; b++) a += (double)dz[(size_t)b * ENS + h] * (double)relu[((size_t)b * ENS + h) * ENS_NN + tid];
    } else if (tid == 16) {
        for (int b = b0; b < b0 + ENS_CHUNK; b++) a += (double)dz[(size_t)b * ENS + h];
    } else if (tid == 17) {
        for (int b = b0; b < b0 + ENS_CHUNK; b++)
            for (int s = 0; s < ENS_NN; s++) a += (double)dconv[((size_t)b * ENS + h) * ENS_NN + s];
    } else if (tid == 18 && h == 0) {
        for (int i = b0 * ENS; i < (b0 + ENS_CHUNK) * ENS; i++) a += (double)err2[i];
    }
    small[((size_t)chunk * ENS + h) * ENS_SMALL + tid] = a;
}

__global__ __launch_bounds__(256) void ens_bwd_finish_kernel(const double* __restrict__ part, const double* __restrict__ small, int batch,
                                                             float* __restrict__ G, float* __restrict__ loss) {
    const int h = blockIdx.x, tid = threadIdx.x, chunks = batch / ENS_CHUNK;
    double g = 0.0;
    for (int k = 0; k < chunks; k++) g += part[((size_t)k * ENS + h) * FILTERS + tid];
    G[ENS_CW + h * FILTERS + tid] = (float)g;
    if (tid > 18) return;
    double a = 0.0;
    for (int k = 0; k < chunks; k++) a += small[((size_t)k * ENS + h) * ENS_SMALL + tid];
    if (tid < ENS_NN) G[ENS_LW + h * ENS_NN + tid] = (float)a;
    else if (tid == 16) G[ENS_LB + h] = (float)a;
    else if (tid == 17) G[ENS_CB + h] = (float)a;
    else if (h == 0) loss[0] = (float)(a / (double)(batch * ENS));
}

// ------------------------------------------------------------------------------------------------
// RND distillation (net5.rs:114-148, 193-204; learn/src/main.rs:404): predictor and frozen target MLP 800 -> 1024 -> 1024 -> 512 on
// x / sum(x^2), raw = |learning - target|^2 per position, loss_rnd = mean(raw), backward through the predictor only.  The linear
// weights are kept like conv weights, [K = in (800 padded to 832)][N = out], so every contraction is gemm() above; what follows is
// the rest of the chain.  Every sum has a fixed order.
constexpr int RND_IN = 800, RND_INP = 832, RND_HID = 1024, RND_OUT = 512;

// x / sum(x^2) of one board (one wave), written in the order of the reference's view of the NCHW planes: column = channel * 25 +
// square (x0 is NHWC); columns 800 .. 831, the K padding, are zero.
__global__ __launch_bounds__(64) void rnd_input_kernel(const float* __restrict__ x0, float* __restrict__ xr) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const float* x = x0 + (size_t)b * RND_IN;
    float s = 0.f;
    for (int i = lane; i < RND_IN; i += 64) s += x[i] * x[i];
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    s = __shfl(s, 0);
    float* y = xr + (size_t)b * RND_INP;
    for (int i = lane; i < RND_INP; i += 64) {
        const int c = i / 25, sq = i - c * 25;
        y[i] = i < RND_IN ? x[sq * 32 + c] / s : 0.f;
    }
}

// h = relu(h) in place (the bias is added by the GEMM's epilogue)
__global__ void rnd_relu_kernel(float* __restrict__ h, size_t total) {
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= total) return;
    float4 v = *(float4*)(h + i);
    v.x = fmaxf(v.x, 0.f);
    v.y = fmaxf(v.y, 0.f);
    v.z = fmaxf(v.z, 0.f);
    v.w = fmaxf(v.w, 0.f);
    *(float4*)(h + i) = v;
}

// d = d * (h > 0) in place: ReLU's derivative is zero where the stored activation is zero, as in the trunk
__global__ void rnd_relu_bwd_kernel(float* __restrict__ d, const float* __restrict__ h, size_t total) {
    const size_t i = ((size_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
    if (i >= total) return;
    float4 v = *(float4*)(d + i);
    const float4 a = *(const float4*)(h + i);
    v.x = a.x > 0.f ? v.x : 0.f;
    v.y = a.y > 0.f ? v.y : 0.f;
    v.z = a.z > 0.f ? v.z : 0.f;
    v.w = a.w > 0.f ? v.w : 0.f;
    *(float4*)(d + i) = v;
}

// raw[b] = sum_j (learning[b][j] - target[b][j])^2 (net5.rs:203) and, when asked for, dY = 2 (learning - target) / batch.
// One workgroup per position, two columns per thread, a fixed tree over the 256 partial sums.
__global__ __launch_bounds__(256) void rnd_distance_kernel(const float* __restrict__ learning, const float* __restrict__ target,
                                                           int batch, float* __restrict__ raw, float* __restrict__ dY) {
    __shared__ float red[256];
    const int b = blockIdx.x, t = threadIdx.x;
    const size_t i0 = (size_t)b * RND_OUT + t, i1 = i0 + 256;
    const float d0 = learning[i0] - target[i0], d1 = learning[i1] - target[i1];
    if (dY) {
        dY[i0] = 2.f * d0 / (float)batch;
        dY[i1] = 2.f * d1 / (float)batch;
    }
    red[t] = d0 * d0 + d1 * d1;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) raw[b] = red[0];
}

// loss_rnd = mean over the batch, in position order
__global__ void rnd_loss_kernel(const float* __restrict__ raw, int batch, float* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double s = 0.0;
    for (int b = 0; b < batch; b++) s += raw[b];
    out[0] = (float)(s / batch);
}

// out[0] = min, out[1] = max of raw[0 .. count)
__global__ __launch_bounds__(256) void rnd_minmax_kernel(const float* __restrict__ raw, int count, float* __restrict__ out) {
    __shared__ float lo[256], hi[256];
    const int t = threadIdx.x;
    float a = INFINITY, b = -INFINITY;
    for (int i = t; i < count; i += 256) {
        a = fminf(a, raw[i]);
        b = fmaxf(b, raw[i]);
    }
    lo[t] = a;
    hi[t] = b;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
            lo[t] = fminf(lo[t], lo[t + o]);
            hi[t] = fmaxf(hi[t], hi[t + o]);
        }
        __syncthreads();
    }
    if (t == 0) {
        out[0] = lo[0];
        out[1] = hi[0];
    }
}

// out[C][R] = in[R][C]^T, R and C multiples of 32: the weight matrix of a linear layer's data gradient
__global__ __launch_bounds__(256) void rnd_transpose_kernel(const float* __restrict__ in, float* __restrict__ out, int R, int C) {
    __shared__ float tile[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int i = ty; i < 32; i += 8) tile[i][tx] = in[(size_t)(r0 + i) * C + c0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8) out[(size_t)(c0 + i) * R + r0 + tx] = tile[tx][i];
}

// ------------------------------------------------------------------------------------------------
struct Param {
    std::string name;
    size_t off = 0, slots = 0;     // offset / extent in the arenas (multiple of 1024)
    int kind = 0;                  // 0 vector as is, 1 conv weight [co][ci][3][3] <-> GEMM layout, 2 buffer (not trained)
    int co = 0, ci = 0, ld = 0, kp = 0;
    size_t count = 0;              // elements in the reference's tensor
    int group = 0;
};

// The RND side of a net5 trainer, allocated when tz_trainer_rnd_enable first switches it on.  The six tensors of one MLP lie in one
// arena at off[]: input_linear.weight [832][1024], .bias, hidden_linear.weight [1024][1024], .bias, final_linear.weight [1024][512],
// .bias.  The predictor has the four arenas of the trunk (parameters, gradients, two moments), the target its parameters only.
struct RndLayer {
    const char* name;
    int in, inp, out;
};
const RndLayer RND_LAYERS[3] = {{"input_linear", RND_IN, RND_INP, RND_HID}, {"hidden_linear", RND_HID, RND_HID, RND_HID},
                                {"final_linear", RND_HID, RND_HID, RND_OUT}};
struct Rnd {
    bool allocated = false, on = false;
    int t_rnd = 0;
    size_t off[6] = {0, 0, 0, 0, 0, 0}, slots[6] = {0, 0, 0, 0, 0, 0}, total = 0;
    float *P = nullptr, *G = nullptr, *M1 = nullptr, *M2 = nullptr, *T = nullptr;
    uint8_t* group = nullptr;
    float* xr = nullptr;                                   // [batch][832]
    float* h[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};   // [learning, target][layer]: [batch][1024] after ReLU
    float* out[2] = {nullptr, nullptr};                    // [batch][512]
    float *dY = nullptr, *dH2 = nullptr, *dH1 = nullptr;   // gradients at the three layers' outputs
    float *w2t = nullptr, *w3t = nullptr;                  // hidden / final weights transposed, for the data gradients
    float *raw = nullptr, *loss = nullptr, *raw_cal = nullptr, *minmax = nullptr, *ws = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev_x0 = nullptr, ev_done = nullptr;
    float last_loss = 0.f;
    bool have_last = false;
};

// The ensemble side of a net4_ensemble trainer, allocated when tz_trainer_set_ensemble_targets first arms it.  While armed the device
// holds the current `ensemble head i.*`; ens_download brings them to the carried variables before anything reads those.
struct Ens {
    bool allocated = false, armed = false, have_last = false;
    int t_ens = 0;
    float *P = nullptr, *G = nullptr, *M1 = nullptr, *M2 = nullptr;
    uint8_t* group = nullptr;
    float *targets = nullptr, *values = nullptr, *relu = nullptr, *dz = nullptr, *dconv = nullptr, *err2 = nullptr, *loss = nullptr;
    double *part = nullptr, *small = nullptr;   // ens_bwd_kernel's per-chunk sums
    float last_loss = 0.f;
};

}  // namespace

struct tz_trainer {
    int arch = 0, n = 0, nn = 0, blocks = 0, batch = 0, M = 0, device = 0;
    int cin = 0, kp_in = 0, pol_ch = 0, np = 0, layers = 0;
    float lr = 1e-4f;
    int t_main = 0, t_ube = 0;
    std::vector<Param> params;
    std::map<std::string, int> index;
    size_t total = 0;
    float *P = nullptr, *G = nullptr, *M1 = nullptr, *M2 = nullptr;
    uint8_t* group_dev = nullptr;
    // activations of one step
    tz_state* states = nullptr;
    float* x0 = nullptr;                 // [M][cin]
    std::vector<float*> c, a;            // per conv layer: pre-BN output, post-activation output  [M][256]
    float* stats = nullptr;              // [layers][2][256] mean, invstd
    double* partial = nullptr;           // [SPLITS][256][2]
    float *mean_dy = nullptr, *mean_dyx = nullptr;
    float* wmirror = nullptr;            // [layers][max K'][256]: slot l - 1 for trunk layer l, the last for the policy conv (mirror_all)
    int kmax = 0;
    hipEvent_t ev_mirror = nullptr;
    float *dA = nullptr, *dB = nullptr, *dC = nullptr, *dskip = nullptr;  // [M][256] gradient ping-pong
    float *pol = nullptr, *dpol = nullptr;                                // [M][np]
    float *pre = nullptr, *value = nullptr, *ube = nullptr;
    float *tpol = nullptr, *tv = nullptr, *tu = nullptr;
    uint8_t* mask = nullptr;
    float *part = nullptr, *loss_p = nullptr, *loss_v = nullptr, *loss_u = nullptr, *losses = nullptr;
    int pstride = 0;
    hipStream_t stream = nullptr;
    // weight gradients run on a second stream beside the data-gradient chain (two dC slots)
    hipStream_t stream2 = nullptr;
    hipEvent_t ev_dc[2] = {nullptr, nullptr}, ev_w[2] = {nullptr, nullptr};
    float* dC2 = nullptr;
    // stream-K GEMMs: workgroups per launch (two per CU) and, per stream, two 64x64 slots per workgroup for partial tiles
    int sk_groups = 512;
    float* sk_ws[2] = {nullptr, nullptr};
    std::vector<void*> allocs;
    // variables of the VarStore the trunk's step never touches (RND nets, SimHash matrix, lcghash_init): carried through save / load.  While RND
    // training is enabled the device holds the current rnd_learning.*; rnd_download brings them here before anything reads them.
    TensorStore extra;
    Rnd rnd;
    Ens ens;
    Rnd4Learn* rnd4 = nullptr;   // net4_rnd's predictor tower (tz_learn_rnd4.h), created when tz_trainer_rnd4_enable first switches it on
};

namespace {

int add_param(tz_trainer* t, const std::string& name, int kind, size_t count, int group, int co = 0, int ci = 0) {
    Param p;
    p.name = name;
    p.kind = kind;
    p.count = count;
    p.group = group;
    size_t elems = count;
    if (kind == 1) {
        p.co = co;
        p.ci = ci;
        p.ld = (co + 63) / 64 * 64;
        p.kp = (9 * ci + 63) / 64 * 64;  // K of the forward GEMM and M of the weight-gradient GEMM
        elems = (size_t)p.kp * p.ld;
    } else if (name.find("policy.conv2d.bias") != std::string::npos) {
        elems = (size_t)(count + 63) / 64 * 64;
    }
    p.slots = (elems + 1023) / 1024 * 1024;
    p.off = t->total;
    t->total += p.slots;
    t->index[name] = (int)t->params.size();
    t->params.push_back(p);
    return TZ_OK;
}

template <typename T>
int dalloc(tz_trainer* t, T** p, size_t count) {
    void* q = nullptr;
    if (hipMalloc(&q, count * sizeof(T)) != hipSuccess) return tz_fail(TZ_ENOMEM, "trainer: device allocation failed");
    if (hipMemset(q, 0, count * sizeof(T)) != hipSuccess) return tz_fail(TZ_EDEVICE, "trainer: memset failed");
    t->allocs.push_back(q);
    *p = (T*)q;
    return TZ_OK;
}

const Param& par(const tz_trainer* t, const std::string& name) { return t->params[t->index.at(name)]; }
float* pp(const tz_trainer* t, const std::string& name) { return t->P + par(t, name).off; }
float* gp(const tz_trainer* t, const std::string& name) { return t->G + par(t, name).off; }

std::string conv_name(const tz_trainer* t, int layer) {
    if (layer == 0) return "core.input_conv2d";
    const int b = (layer - 1) / 2;
    return "core.res_block_" + std::to_string(b) + ((layer - 1) % 2 ? ".b" : ".a") + ".conv2d";
}
std::string bn_name(const tz_trainer* t, int layer) {
    if (layer == 0) return "core.batch_norm";
    const int b = (layer - 1) / 2;
    return "core.res_block_" + std::to_string(b) + ((layer - 1) % 2 ? ".b" : ".a") + ".batch_norm";
}

int launch_check(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return tz_fail(TZ_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
    return TZ_OK;
}

int gemm(tz_trainer* t, bool at, const float* A, const float* B, float* C, const float* bias, int M, int N, int K, int lda,
         int ldb, int ldc, bool accumulate, hipStream_t st = nullptr, int gather_c = 0) {
    if (!st) st = t->stream;
    if (M % 64 || N % 64 || K % 32 || lda % 4 || ldb % 4 || ldc % 4 || gather_c % 4 || (long long)(M / 64) * (N / 64) * (K / 32) > (1ll << 22))
        return tz_fail(TZ_EINVAL, "trainer gemm: unaligned shape");
    const int acc = accumulate ? 1 : 0;
    static const bool tiled = getenv("TZ_LEARN_GEMM") && !strcmp(getenv("TZ_LEARN_GEMM"), "tile");   // A/B: one workgroup per tile
    if (!tiled) {
        const int tiles_m = M / 64, tiles = tiles_m * (N / 64), S = K / 32;
        const long long total = (long long)tiles * S;
        const int G = (int)std::min<long long>(total, t->sk_groups);
        float* ws = st == t->stream2 ? t->sk_ws[1] : (t->rnd.stream && st == t->rnd.stream) ? t->rnd.ws : t->sk_ws[0];
        const int gn = gather_c ? t->n : 0;
        if (gather_c && at)
            gemm_sk_kernel<true, true><<<G, 256, 0, st>>>(A, B, C, bias, K, lda, ldb, ldc, acc, gn, gather_c, tiles_m, total, ws);
        else if (gather_c)
            gemm_sk_kernel<false, true><<<G, 256, 0, st>>>(A, B, C, bias, K, lda, ldb, ldc, acc, gn, gather_c, tiles_m, total, ws);
        else if (at)
            gemm_sk_kernel<true, false><<<G, 256, 0, st>>>(A, B, C, bias, K, lda, ldb, ldc, acc, 0, 0, tiles_m, total, ws);
        else
            gemm_sk_kernel<false, false><<<G, 256, 0, st>>>(A, B, C, bias, K, lda, ldb, ldc, acc, 0, 0, tiles_m, total, ws);
        if (total % G || (total / G) % S)   // some tile is shared between workgroups
            gemm_fixup_kernel<<<tiles, 256, 0, st>>>(C, bias, S, ldc, acc, tiles_m, (unsigned)total, (unsigned)G, ws);
        return launch_check("gemm_sk");
    }
    const dim3 grid(M / 64, N / 64);
    if (gather_c) {   // A = im2col view of the NHWC tensor at `A` with gather_c channels
        if (at)
            gemm_f32_kernel<true, true><<<grid, 512, 0, st>>>(A, B, C, bias, K, lda, ldb, ldc, acc, t->n, gather_c);
        else
            gemm_f32_kernel<false, true><<<grid, 512, 0, st>>>(A, B, C, bias, K, lda, ldb, ldc, acc, t->n, gather_c);
    } else if (at) {
        gemm_f32_kernel<true, false><<<grid, 512, 0, st>>>(A, B, C, bias, K, lda, ldb, ldc, acc, 0, 0);
    } else {
        gemm_f32_kernel<false, false><<<grid, 512, 0, st>>>(A, B, C, bias, K, lda, ldb, ldc, acc, 0, 0);
    }
    return launch_check("gemm_f32");
}

int forward(tz_trainer* t) {
    int rc;
    const int M = t->M;
    const size_t act = (size_t)M * FILTERS;
    if ((rc = tz_nn_encode_planes(t->n, t->cin, t->states, t->batch, t->x0, t->stream))) return rc;
    if (t->rnd.on) TZ_HIP(hipEventRecord(t->rnd.ev_x0, t->stream));   // the RND chain starts from the planes, beside the trunk
    if (t->rnd4 && t->rnd4->on) TZ_HIP(hipEventRecord(t->rnd4->ev_x0, t->stream));
    for (int l = 0; l < t->layers; l++) {
        const float* in = l == 0 ? t->x0 : t->a[l - 1];
        const int C = l == 0 ? t->cin : FILTERS, Kp = l == 0 ? t->kp_in : 9 * FILTERS;
        if ((rc = gemm(t, false, in, pp(t, conv_name(t, l) + ".weight"), t->c[l], nullptr, M, FILTERS, Kp, Kp, FILTERS,
                       FILTERS, false, nullptr, C)))
            return rc;
        float* mean = t->stats + (size_t)l * 2 * FILTERS;
        float* invstd = mean + FILTERS;
        const std::string bn = bn_name(t, l);
        column_partials_kernel<<<dim3(FILTERS / 32, SPLITS), 256, 0, t->stream>>>(0, t->c[l], nullptr, nullptr, nullptr,
                                                                                  nullptr, M, t->partial);
        bn_stats_finish_kernel<<<1, FILTERS, 0, t->stream>>>(t->partial, M, mean, invstd, pp(t, bn + ".running_mean"),
                                                             pp(t, bn + ".running_var"));
        const float* skip = (l > 0 && (l - 1) % 2 == 1) ? (l == 2 ? t->a[0] : t->a[l - 2]) : nullptr;
        bn_apply_kernel<<<(unsigned)((act / 4 + 255) / 256), 256, 0, t->stream>>>(
            t->c[l], mean, invstd, pp(t, bn + ".weight"), pp(t, bn + ".bias"), skip, t->a[l], act);
        if ((rc = launch_check("batch norm forward"))) return rc;
    }
    const float* T = t->a[t->layers - 1];
    if ((rc = gemm(t, false, T, pp(t, "policy.conv2d.weight"), t->pol, pp(t, "policy.conv2d.bias"), M, t->np,
                   9 * FILTERS, 9 * FILTERS, t->np, t->np, false, nullptr, FILTERS)))
        return rc;
    heads_fwd_kernel<<<t->batch, 64, 0, t->stream>>>(T, pp(t, "value.conv2d.weight"), pp(t, "value.conv2d.bias"),
                                                    pp(t, "value.linear.weight"), pp(t, "value.linear.bias"),
                                                    pp(t, "ube.conv2d.weight"), pp(t, "ube.conv2d.bias"),
                                                    pp(t, "ube.linear.weight"), pp(t, "ube.linear.bias"), t->nn, t->pre, M,
                                                    t->value, t->ube);
    return launch_check("heads forward");
}

// data gradient of a 3x3 conv: out[M][256] (+)= im2col(dc [M][Cd]) x mirror(W); `wm` = the mirrored matrix (mirror_all)
int conv_dgrad(tz_trainer* t, const float* dc, int Cd, const float* wm, float* out, bool accumulate) {
    return gemm(t, false, dc, wm, out, nullptr, t->M, FILTERS, 9 * Cd, 9 * Cd, FILTERS, FILTERS, accumulate, nullptr, Cd);
}

// The mirrored weight matrices of every data gradient of the step (trunk layers 1 .., slot l - 1; the policy conv in the last slot),
// built on the second stream while the forward pass runs on the first: they depend on the weights only, and one small launch ahead of
// each of the 41 data-gradient GEMMs was 0.26 ms of the main stream's critical path.
int mirror_all(tz_trainer* t) {
    const size_t slot = (size_t)t->kmax * FILTERS;
    for (int l = 1; l <= t->layers; l++) {
        const bool policy = l == t->layers;
        const int Cd = policy ? t->np : FILTERS;
        const float* W = pp(t, policy ? std::string("policy.conv2d.weight") : conv_name(t, l) + ".weight");
        const size_t total = (size_t)9 * Cd * FILTERS;
        mirror_weights_kernel<<<(unsigned)((total + 255) / 256), 256, 0, t->stream2>>>(W, t->wmirror + (size_t)(l - 1) * slot, FILTERS, Cd, Cd, FILTERS);
    }
    int rc;
    if ((rc = launch_check("mirror weights"))) return rc;
    TZ_HIP(hipEventRecord(t->ev_mirror, t->stream2));
    return TZ_OK;
}

int backward(tz_trainer* t, int train_ube) {
    int rc;
    const int M = t->M, L = t->layers;
    const size_t act = (size_t)M * FILTERS;
    const float* T = t->a[L - 1];
    // losses and the gradients at the three outputs
    policy_loss_kernel<<<t->batch, 256, 0, t->stream>>>(t->pol, t->tpol, t->mask, t->nn, t->pol_ch, t->np, t->batch, t->dpol,
                                                       t->loss_p);
    heads_bwd_kernel<<<t->batch, 64, 0, t->stream>>>(T, pp(t, "value.conv2d.weight"), pp(t, "value.linear.weight"),
                                                    pp(t, "ube.linear.weight"), t->pre, M, t->nn, t->batch, t->value, t->ube,
                                                    t->tv, t->tu, train_ube, t->part, t->pstride, t->dA, t->loss_v,
                                                    t->loss_u);
    losses_kernel<<<1, 1, 0, t->stream>>>(t->loss_p, t->loss_v, t->loss_u, t->batch, t->losses);
    if ((rc = launch_check("losses"))) return rc;
    {   // head parameter gradients: part[b] = [conv w 256 | conv b | lin w nn | lin b] x {value, ube}
        const int hs = FILTERS + 1 + t->nn + 1;
        const char* heads[2] = {"value", "ube"};
        for (int h = 0; h < 2; h++) {
            const float* base = t->part + (size_t)h * hs;
            const std::string p = heads[h];
            sum_rows_kernel<<<1, 256, 0, t->stream>>>(base, t->batch, t->pstride, FILTERS, gp(t, p + ".conv2d.weight"));
            sum_rows_kernel<<<1, 64, 0, t->stream>>>(base + FILTERS, t->batch, t->pstride, 1, gp(t, p + ".conv2d.bias"));
            sum_rows_kernel<<<1, 64, 0, t->stream>>>(base + FILTERS + 1, t->batch, t->pstride, t->nn, gp(t, p + ".linear.weight"));
            sum_rows_kernel<<<1, 64, 0, t->stream>>>(base + FILTERS + 1 + t->nn, t->batch, t->pstride, 1, gp(t, p + ".linear.bias"));
        }
        if ((rc = launch_check("head gradients"))) return rc;
    }
    // policy conv: weight / bias gradient, and its data gradient added to the value head's (already in dA)
    if ((rc = gemm(t, true, T, t->dpol, gp(t, "policy.conv2d.weight"), nullptr, 9 * FILTERS, t->np, M, 9 * FILTERS, t->np,
                   t->np, false, nullptr, FILTERS)))
        return rc;
    column_sum_kernel<<<(t->np + 31) / 32, 256, 0, t->stream>>>(t->dpol, M, t->np, t->np, gp(t, "policy.conv2d.bias"));
    if ((rc = launch_check("policy bias gradient"))) return rc;
    TZ_HIP(hipStreamWaitEvent(t->stream, t->ev_mirror, 0));
    if ((rc = conv_dgrad(t, t->dpol, t->np, t->wmirror + (size_t)(t->layers - 1) * t->kmax * FILTERS, t->dA, true))) return rc;
    // trunk, last layer first.  `da` = gradient w.r.t. a[l]; three [M][256] buffers rotate between the roles
    // "gradient coming in", "gradient of the skip connection" and "gradient going out".
    float* bufs[3] = {t->dA, t->dB, t->dskip};
    float* da = t->dA;
    float* skip = nullptr;
    auto free_buf = [&](const float* x, const float* y) {
        for (float* b : bufs)
            if (b != x && b != y) return b;
        return (float*)nullptr;
    };
    // events of this step only: the previous step ended with the main stream waiting for both (below), and a wait for an event that
    // was recorded outside a stream capture has no place in the captured graph
    bool recorded[2] = {false, false};
    for (int l = L - 1; l >= 0; l--) {
        const bool second = l > 0 && (l - 1) % 2 == 1;  // second SmallBlock of a residual block: output joins the skip
        const float* mean = t->stats + (size_t)l * 2 * FILTERS;
        const float* invstd = mean + FILTERS;
        const std::string bn = bn_name(t, l), cv = conv_name(t, l);
        if (second) skip = free_buf(da, nullptr);
        const int slot = l & 1;
        float* dc = slot ? t->dC2 : t->dC;
        if (recorded[slot]) TZ_HIP(hipStreamWaitEvent(t->stream, t->ev_w[slot], 0));  // the weight gradient of layer l+2 has read this slot
        column_partials_kernel<<<dim3(FILTERS / 32, SPLITS), 256, 0, t->stream>>>(1, t->c[l], da, t->a[l], mean, invstd, M,
                                                                                  t->partial);
        bn_bwd_finish_kernel<<<1, FILTERS, 0, t->stream>>>(t->partial, M, gp(t, bn + ".weight"), gp(t, bn + ".bias"),
                                                           t->mean_dy, t->mean_dyx);
        bn_bwd_apply_kernel<<<(unsigned)((act + 255) / 256), 256, 0, t->stream>>>(
            t->c[l], da, t->a[l], mean, invstd, pp(t, bn + ".weight"), t->mean_dy, t->mean_dyx, dc,
            second ? skip : nullptr, act);
        if ((rc = launch_check("batch norm backward"))) return rc;
        TZ_HIP(hipEventRecord(t->ev_dc[slot], t->stream));
        // weight gradient on the second stream: dW = im2col(input)^T x dc
        const float* in = l == 0 ? t->x0 : t->a[l - 1];
        const int C = l == 0 ? t->cin : FILTERS, Kp = l == 0 ? t->kp_in : 9 * FILTERS;
        TZ_HIP(hipStreamWaitEvent(t->stream2, t->ev_dc[slot], 0));
        if ((rc = gemm(t, true, in, dc, gp(t, cv + ".weight"), nullptr, Kp, FILTERS, M, Kp, FILTERS, FILTERS, false,
                       t->stream2, C)))
            return rc;
        TZ_HIP(hipEventRecord(t->ev_w[slot], t->stream2));
        recorded[slot] = true;
        if (l == 0) break;
        if (second) {  // gradient w.r.t. a[l-1] (the ReLU between the two SmallBlocks)
            float* out = free_buf(da, skip);
            if ((rc = conv_dgrad(t, dc, FILTERS, t->wmirror + (size_t)(l - 1) * t->kmax * FILTERS, out, false))) return rc;
            da = out;
        } else {       // gradient w.r.t. the block input: through the first SmallBlock plus the skip connection
            if ((rc = conv_dgrad(t, dc, FILTERS, t->wmirror + (size_t)(l - 1) * t->kmax * FILTERS, skip, true))) return rc;
            da = skip;
            skip = nullptr;
        }
    }
    // every weight gradient is in place before anything else (Adam, a read-back) runs on the main stream
    for (int slot = 0; slot < 2; slot++)
        if (recorded[slot]) TZ_HIP(hipStreamWaitEvent(t->stream, t->ev_w[slot], 0));
    return TZ_OK;
}

// ---- RND chain ----
const float* rnd_bias(const Rnd& r, const float* arena, int layer) { return arena + r.off[2 * layer + 1]; }

// both MLPs on the planes in t->x0 (batch boards): xr, h[net][0], h[net][1], out[net]
int rnd_forward(tz_trainer* t, hipStream_t st) {
    Rnd& r = t->rnd;
    const int B = t->batch;
    int rc;
    rnd_input_kernel<<<B, 64, 0, st>>>(t->x0, r.xr);
    if ((rc = launch_check("rnd input"))) return rc;
    const size_t hid = (size_t)B * RND_HID;
    for (int net = 0; net < 2; net++) {
        const float* W = net == 0 ? r.P : r.T;
        if ((rc = gemm(t, false, r.xr, W + r.off[0], r.h[net][0], rnd_bias(r, W, 0), B, RND_HID, RND_INP, RND_INP, RND_HID, RND_HID, false, st)))
            return rc;
        rnd_relu_kernel<<<(unsigned)((hid / 4 + 255) / 256), 256, 0, st>>>(r.h[net][0], hid);
        if ((rc = gemm(t, false, r.h[net][0], W + r.off[2], r.h[net][1], rnd_bias(r, W, 1), B, RND_HID, RND_HID, RND_HID, RND_HID, RND_HID, false, st)))
            return rc;
        rnd_relu_kernel<<<(unsigned)((hid / 4 + 255) / 256), 256, 0, st>>>(r.h[net][1], hid);
        if ((rc = gemm(t, false, r.h[net][1], W + r.off[4], r.out[net], rnd_bias(r, W, 2), B, RND_OUT, RND_HID, RND_HID, RND_OUT, RND_OUT, false, st)))
            return rc;
    }
    return launch_check("rnd forward");
}

// The whole distillation step on the RND stream: it waits for the planes only, so it runs beside the trunk's forward; the main stream
// joins it (ev_done) before its own Adam launch.
int rnd_chain(tz_trainer* t, int apply_step) {
    Rnd& r = t->rnd;
    const int B = t->batch;
    hipStream_t st = r.stream;
    int rc;
    // the transposed weights of the two data gradients depend on the weights only: ahead of the wait for the planes
    rnd_transpose_kernel<<<dim3(RND_OUT / 32, RND_HID / 32), 256, 0, st>>>(r.P + r.off[4], r.w3t, RND_HID, RND_OUT);
    rnd_transpose_kernel<<<dim3(RND_HID / 32, RND_HID / 32), 256, 0, st>>>(r.P + r.off[2], r.w2t, RND_HID, RND_HID);
    if ((rc = launch_check("rnd transpose"))) return rc;
    TZ_HIP(hipStreamWaitEvent(st, r.ev_x0, 0));
    if ((rc = rnd_forward(t, st))) return rc;
    rnd_distance_kernel<<<B, 256, 0, st>>>(r.out[0], r.out[1], B, r.raw, r.dY);
    rnd_loss_kernel<<<1, 1, 0, st>>>(r.raw, B, r.loss);
    if ((rc = launch_check("rnd loss"))) return rc;
    const size_t hid = (size_t)B * RND_HID;
    const unsigned hid_blocks = (unsigned)((hid / 4 + 255) / 256);
    // final layer: dW = h2^T x dY, db = column sums of dY, dH2 = dY x W^T masked by h2 > 0
    if ((rc = gemm(t, true, r.h[0][1], r.dY, r.G + r.off[4], nullptr, RND_HID, RND_OUT, B, RND_HID, RND_OUT, RND_OUT, false, st))) return rc;
    column_sum_kernel<<<RND_OUT / 32, 256, 0, st>>>(r.dY, B, RND_OUT, RND_OUT, r.G + r.off[5]);
    if ((rc = gemm(t, false, r.dY, r.w3t, r.dH2, nullptr, B, RND_HID, RND_OUT, RND_OUT, RND_HID, RND_HID, false, st))) return rc;
    rnd_relu_bwd_kernel<<<hid_blocks, 256, 0, st>>>(r.dH2, r.h[0][1], hid);
    // hidden layer
    if ((rc = gemm(t, true, r.h[0][0], r.dH2, r.G + r.off[2], nullptr, RND_HID, RND_HID, B, RND_HID, RND_HID, RND_HID, false, st))) return rc;
    column_sum_kernel<<<RND_HID / 32, 256, 0, st>>>(r.dH2, B, RND_HID, RND_HID, r.G + r.off[3]);
    if ((rc = gemm(t, false, r.dH2, r.w2t, r.dH1, nullptr, B, RND_HID, RND_HID, RND_HID, RND_HID, RND_HID, false, st))) return rc;
    rnd_relu_bwd_kernel<<<hid_blocks, 256, 0, st>>>(r.dH1, r.h[0][0], hid);
    // input layer: the gradient comes out in the weights' own layout [832][1024]; its padding rows are xr's zero columns times dH1
    if ((rc = gemm(t, true, r.xr, r.dH1, r.G + r.off[0], nullptr, RND_INP, RND_HID, B, RND_INP, RND_HID, RND_HID, false, st))) return rc;
    column_sum_kernel<<<RND_HID / 32, 256, 0, st>>>(r.dH1, B, RND_HID, RND_HID, r.G + r.off[1]);
    if ((rc = launch_check("rnd backward"))) return rc;
    if (apply_step) {
        r.t_rnd++;
        adam_kernel<<<(unsigned)(r.total / 1024), 256, 0, st>>>(r.P, r.G, r.M1, r.M2, r.group, t->lr, 0, 0, r.t_rnd);
        if ((rc = launch_check("rnd adam"))) return rc;
    }
    TZ_HIP(hipEventRecord(r.ev_done, st));
    return TZ_OK;
}

// index 0 .. 5 of an rnd_learning.* variable in the arena, -1 for any other name
int rnd_index(const std::string& name, const char* net = "rnd_learning") {
    for (int l = 0; l < 3; l++)
        for (int part = 0; part < 2; part++)
            if (name == std::string(net) + "." + RND_LAYERS[l].name + (part ? ".bias" : ".weight")) return 2 * l + part;
    return -1;
}
std::string rnd_name(const char* net, int i) { return std::string(net) + "." + RND_LAYERS[i / 2].name + (i % 2 ? ".bias" : ".weight"); }
size_t rnd_count(int i) { return i % 2 ? (size_t)RND_LAYERS[i / 2].out : (size_t)RND_LAYERS[i / 2].out * RND_LAYERS[i / 2].in; }

// reference layout ([out][in] weights, biases as they are) <-> the arena's ([in, padded][out], padding zero)
void rnd_pack(int i, const float* data, std::vector<float>& host, size_t slots) {
    const RndLayer& L = RND_LAYERS[i / 2];
    host.assign(slots, 0.f);
    if (i % 2) {
        memcpy(host.data(), data, sizeof(float) * L.out);
        return;
    }
    for (int o = 0; o < L.out; o++)
        for (int k = 0; k < L.in; k++) host[(size_t)k * L.out + o] = data[(size_t)o * L.in + k];
}
void rnd_unpack(int i, const std::vector<float>& host, float* out) {
    const RndLayer& L = RND_LAYERS[i / 2];
    if (i % 2) {
        memcpy(out, host.data(), sizeof(float) * L.out);
        return;
    }
    for (int o = 0; o < L.out; o++)
        for (int k = 0; k < L.in; k++) out[(size_t)o * L.in + k] = host[(size_t)k * L.out + o];
}

bool rnd_variables_present(const tz_trainer* t) {
    for (const char* net : {"rnd_learning", "rnd_target"})
        for (int i = 0; i < 6; i++) {
            auto it = t->extra.find(rnd_name(net, i));
            if (it == t->extra.end() || it->second.data.size() != rnd_count(i)) return false;
        }
    for (const char* v : {"min", "max"}) {
        auto it = t->extra.find(v);
        if (it == t->extra.end() || it->second.data.size() != 1) return false;
    }
    return true;
}

// the carried rnd_learning.* / rnd_target.* go to the device (parameters only: gradients and moments stay)
int rnd_upload(tz_trainer* t) {
    Rnd& r = t->rnd;
    std::vector<float> host;
    TZ_HIP(hipStreamSynchronize(t->stream));
    TZ_HIP(hipStreamSynchronize(r.stream));
    for (int net = 0; net < 2; net++)
        for (int i = 0; i < 6; i++) {
            rnd_pack(i, t->extra.at(rnd_name(net ? "rnd_target" : "rnd_learning", i)).data.data(), host, r.slots[i]);
            TZ_HIP(hipMemcpy((net ? r.T : r.P) + r.off[i], host.data(), r.slots[i] * sizeof(float), hipMemcpyHostToDevice));
        }
    return TZ_OK;
}

// ... and the current predictor comes back into the carried variables
int rnd_download(tz_trainer* t) {
    Rnd& r = t->rnd;
    TZ_HIP(hipSetDevice(t->device));
    TZ_HIP(hipStreamSynchronize(t->stream));
    TZ_HIP(hipStreamSynchronize(r.stream));
    std::vector<float> host;
    for (int i = 0; i < 6; i++) {
        host.resize(r.slots[i]);
        TZ_HIP(hipMemcpy(host.data(), r.P + r.off[i], r.slots[i] * sizeof(float), hipMemcpyDeviceToHost));
        HostTensor& h = t->extra[rnd_name("rnd_learning", i)];
        h.data.resize(rnd_count(i));
        rnd_unpack(i, host, h.data.data());
    }
    return TZ_OK;
}

int rnd_allocate(tz_trainer* t) {
    Rnd& r = t->rnd;
    if (r.allocated) return TZ_OK;
    r.total = 0;
    for (int i = 0; i < 6; i++) {
        const RndLayer& L = RND_LAYERS[i / 2];
        const size_t elems = i % 2 ? (size_t)L.out : (size_t)L.inp * L.out;
        r.slots[i] = (elems + 1023) / 1024 * 1024;
        r.off[i] = r.total;
        r.total += r.slots[i];
    }
    const size_t B = (size_t)t->batch;
    int rc;
    if ((rc = dalloc(t, &r.P, r.total)) || (rc = dalloc(t, &r.G, r.total)) || (rc = dalloc(t, &r.M1, r.total)) ||
        (rc = dalloc(t, &r.M2, r.total)) || (rc = dalloc(t, &r.T, r.total)) || (rc = dalloc(t, &r.group, r.total / 1024)) ||
        (rc = dalloc(t, &r.xr, B * RND_INP)) || (rc = dalloc(t, &r.out[0], B * RND_OUT)) || (rc = dalloc(t, &r.out[1], B * RND_OUT)) ||
        (rc = dalloc(t, &r.dY, B * RND_OUT)) || (rc = dalloc(t, &r.dH2, B * RND_HID)) || (rc = dalloc(t, &r.dH1, B * RND_HID)) ||
        (rc = dalloc(t, &r.w2t, (size_t)RND_HID * RND_HID)) || (rc = dalloc(t, &r.w3t, (size_t)RND_HID * RND_OUT)) ||
        (rc = dalloc(t, &r.raw, B)) || (rc = dalloc(t, &r.raw_cal, B)) || (rc = dalloc(t, &r.loss, (size_t)4)) ||
        (rc = dalloc(t, &r.minmax, (size_t)4)) || (rc = dalloc(t, &r.ws, (size_t)t->sk_groups * 2 * 4096)))
        return rc;
    for (int net = 0; net < 2; net++)
        for (int l = 0; l < 2; l++)
            if ((rc = dalloc(t, &r.h[net][l], B * RND_HID))) return rc;
    TZ_HIP(hipMemset(r.group, 3, r.total / 1024));
    if (!r.stream) TZ_HIP(hipStreamCreate(&r.stream));
    if (!r.ev_x0) TZ_HIP(hipEventCreateWithFlags(&r.ev_x0, hipEventDisableTiming));
    if (!r.ev_done) TZ_HIP(hipEventCreateWithFlags(&r.ev_done, hipEventDisableTiming));
    r.allocated = true;
    return TZ_OK;
}

// place and size of an `ensemble head i.*` variable in the arena; false for any other name
const char* const ENS_PARTS[4] = {".conv2d.weight", ".conv2d.bias", ".linear.weight", ".linear.bias"};
std::string ens_name(int head, int part) { return "ensemble head " + std::to_string(head) + ENS_PARTS[part]; }
void ens_place(int head, int part, size_t& off, size_t& count) {
    count = part == 0 ? FILTERS : part == 2 ? ENS_NN : 1;
    off = part == 0 ? ENS_CW + (size_t)head * FILTERS : part == 1 ? ENS_CB + head : part == 2 ? ENS_LW + (size_t)head * ENS_NN : ENS_LB + head;
}
bool ens_find(const std::string& name, size_t& off, size_t& count) {
    for (int head = 0; head < ENS; head++)
        for (int part = 0; part < 4; part++)
            if (name == ens_name(head, part)) {
                ens_place(head, part, off, count);
                return true;
            }
    return false;
}
bool ens_variables_present(const tz_trainer* t) {
    for (int head = 0; head < ENS; head++)
        for (int part = 0; part < 4; part++) {
            size_t off, count;
            ens_place(head, part, off, count);
            auto it = t->extra.find(ens_name(head, part));
            if (it == t->extra.end() || it->second.data.size() != count) return false;
        }
    return true;
}
// the carried heads go to the device (parameters only: gradients and moments stay) ...
int ens_upload(tz_trainer* t) {
    std::vector<float> host(ENS_SLOTS, 0.f);
    for (int head = 0; head < ENS; head++)
        for (int part = 0; part < 4; part++) {
            size_t off, count;
            ens_place(head, part, off, count);
            memcpy(host.data() + off, t->extra.at(ens_name(head, part)).data.data(), count * sizeof(float));
        }
    TZ_HIP(hipStreamSynchronize(t->stream));
    TZ_HIP(hipMemcpy(t->ens.P, host.data(), ENS_SLOTS * sizeof(float), hipMemcpyHostToDevice));
    return TZ_OK;
}
// ... and the current ones come back into the carried variables
int ens_download(tz_trainer* t) {
    std::vector<float> host(ENS_SLOTS);
    TZ_HIP(hipSetDevice(t->device));
    TZ_HIP(hipStreamSynchronize(t->stream));
    TZ_HIP(hipMemcpy(host.data(), t->ens.P, ENS_SLOTS * sizeof(float), hipMemcpyDeviceToHost));
    for (int head = 0; head < ENS; head++)
        for (int part = 0; part < 4; part++) {
            size_t off, count;
            ens_place(head, part, off, count);
            HostTensor& h = t->extra[ens_name(head, part)];
            h.data.assign(host.begin() + off, host.begin() + off + count);
        }
    return TZ_OK;
}
int ens_allocate(tz_trainer* t) {
    Ens& e = t->ens;
    if (e.allocated) return TZ_OK;
    const size_t B = (size_t)t->batch;
    int rc;
    if ((rc = dalloc(t, &e.P, (size_t)ENS_SLOTS)) || (rc = dalloc(t, &e.G, (size_t)ENS_SLOTS)) || (rc = dalloc(t, &e.M1, (size_t)ENS_SLOTS)) ||
        (rc = dalloc(t, &e.M2, (size_t)ENS_SLOTS)) || (rc = dalloc(t, &e.group, (size_t)ENS_SLOTS / 1024)) || (rc = dalloc(t, &e.targets, B * ENS)) ||
        (rc = dalloc(t, &e.values, B * ENS)) || (rc = dalloc(t, &e.relu, B * ENS * ENS_NN)) || (rc = dalloc(t, &e.dz, B * ENS)) ||
        (rc = dalloc(t, &e.dconv, B * ENS * ENS_NN)) || (rc = dalloc(t, &e.err2, B * ENS)) || (rc = dalloc(t, &e.loss, (size_t)4)) ||
        (rc = dalloc(t, &e.part, B / ENS_CHUNK * ENS * FILTERS)) || (rc = dalloc(t, &e.small, B / ENS_CHUNK * ENS * ENS_SMALL)))
        return rc;
    TZ_HIP(hipMemset(e.group, 3, ENS_SLOTS / 1024));   // adam_kernel's group of a side arena: the step count passed as t_rnd
    e.allocated = true;
    return TZ_OK;
}
// the armed part of a step, on the step's stream behind its backward: nothing of the step itself is reordered or reads what this writes
int ens_chain(tz_trainer* t, int apply_step) {
    Ens& e = t->ens;
    const float* T = t->a[t->layers - 1];
    ens_fwd_kernel<<<t->batch, 256, 0, t->stream>>>(T, e.P, e.targets, t->batch, e.values, e.relu, e.dz, e.dconv, e.err2);
    ens_bwd_kernel<<<dim3(ENS, t->batch / ENS_CHUNK), 256, 0, t->stream>>>(T, e.relu, e.dz, e.dconv, e.err2, e.part, e.small);
    ens_bwd_finish_kernel<<<ENS, 256, 0, t->stream>>>(e.part, e.small, t->batch, e.G, e.loss);
    int rc;
    if ((rc = launch_check("ensemble heads"))) return rc;
    if (apply_step) {
        e.t_ens++;
        adam_kernel<<<ENS_SLOTS / 1024, 256, 0, t->stream>>>(e.P, e.G, e.M1, e.M2, e.group, t->lr, 0, 0, e.t_ens);
        if ((rc = launch_check("ensemble adam"))) return rc;
    }
    return TZ_OK;
}

// net4_rnd's distillation step on the tower's own stream (tz_learn_rnd4.hip): it waits for the planes only, and nothing of the trunk's
// step reads what it writes; the main stream joins before its own Adam launch.  The predictor's group counts its own Adam steps.
int rnd4_chain(tz_trainer* t, int apply_step) {
    Rnd4Learn* r = t->rnd4;
    int rc;
    if ((rc = tz_rnd4l_chain(r, t->x0, apply_step))) return rc;
    if (apply_step) {
        r->t_step++;
        adam_kernel<<<R4L_TOTAL / 1024, 256, 0, r->stream>>>(r->P, r->G, r->M1, r->M2, r->group, t->lr, 0, 0, r->t_step);
        if ((rc = launch_check("rnd4 adam"))) return rc;
    }
    TZ_HIP(hipEventRecord(r->ev_done, r->stream));
    return TZ_OK;
}
bool rnd4_on(const tz_trainer* t) { return t->rnd4 && t->rnd4->on; }

}  // namespace
// ------------------------------------------------------------------------------------------------
// C ABI (include/takzero_hip.h, "Trainer")
extern "C" {

int tz_trainer_create(int board_n, int arch, int device_id, int blocks, int batch, float learning_rate, tz_trainer** out) {
    if (!out) return tz_fail(TZ_EINVAL, "tz_trainer_create: null out");
    *out = nullptr;
    if (board_n < 3 || board_n > 6) return tz_fail(TZ_EINVAL, "tz_trainer_create: board size must be 3..6");
    if (arch == TZ_ARCH_NET5 && board_n != 5) return tz_fail(TZ_EINVAL, "tz_trainer_create: net5 is a 5x5 network");
    if (arch == TZ_ARCH_NET4_SIMHASH && board_n != 4) return tz_fail(TZ_EINVAL, "tz_trainer_create: net4_simhash is 4x4");
    if (arch == TZ_ARCH_NET6_SIMHASH && board_n != 6) return tz_fail(TZ_EINVAL, "tz_trainer_create: net6_simhash is 6x6");
    if (arch == TZ_ARCH_NET4_LCGHASH && board_n != 4) return tz_fail(TZ_EINVAL, "tz_trainer_create: net4_lcghash is 4x4");
    if (arch == TZ_ARCH_NET4_ENSEMBLE && board_n != 4) return tz_fail(TZ_EINVAL, "tz_trainer_create: net4_ensemble is 4x4");
    if (arch == TZ_ARCH_NET4_RND && board_n != 4) return tz_fail(TZ_EINVAL, "tz_trainer_create: net4_rnd is 4x4");   // its towers, min and max are carried
    if (batch <= 0 || batch % 64) return tz_fail(TZ_EINVAL, "tz_trainer_create: batch must be a positive multiple of 64");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device_id < 0 || device_id >= ndev)
        return tz_fail(TZ_EDEVICE, "tz_trainer_create: no such HIP device (there is no CPU path)");
    TZ_HIP(hipSetDevice(device_id));
    tz_trainer* t = new tz_trainer();
    t->arch = arch;
    t->n = board_n;
    t->nn = board_n * board_n;
    t->device = device_id;
    t->blocks = arch == TZ_ARCH_NET5 ? 20 : arch == TZ_ARCH_TEST ? blocks : 16;
    t->batch = batch;
    t->M = batch * t->nn;
    t->cin = tz_input_channels(board_n);
    t->kp_in = (9 * t->cin + 63) / 64 * 64;
    t->pol_ch = 3 + 4 * ((1 << board_n) - 2);
    t->np = (t->pol_ch + 63) / 64 * 64;
    t->layers = 1 + 2 * t->blocks;
    t->lr = learning_rate;
    int rc = TZ_OK;
    auto bn = [&](const std::string& p) {
        add_param(t, p + ".weight", 0, FILTERS, 1);
        add_param(t, p + ".bias", 0, FILTERS, 1);
        add_param(t, p + ".running_mean", 2, FILTERS, 0);
        add_param(t, p + ".running_var", 2, FILTERS, 0);
    };
    add_param(t, "core.input_conv2d.weight", 1, (size_t)FILTERS * t->cin * 9, 1, FILTERS, t->cin);
    bn("core.batch_norm");
    for (int b = 0; b < t->blocks; b++)
        for (const char* half : {".a", ".b"}) {
            const std::string p = "core.res_block_" + std::to_string(b) + half;
            add_param(t, p + ".conv2d.weight", 1, (size_t)FILTERS * FILTERS * 9, 1, FILTERS, FILTERS);
            bn(p + ".batch_norm");
        }
    add_param(t, "policy.conv2d.weight", 1, (size_t)t->pol_ch * FILTERS * 9, 1, t->pol_ch, FILTERS);
    add_param(t, "policy.conv2d.bias", 0, t->pol_ch, 1);
    for (const char* h : {"value", "ube"}) {
        const int g = std::string(h) == "ube" ? 2 : 1;
        add_param(t, std::string(h) + ".conv2d.weight", 0, FILTERS, g);
        add_param(t, std::string(h) + ".conv2d.bias", 0, 1, g);
        add_param(t, std::string(h) + ".linear.weight", 0, t->nn, g);
        add_param(t, std::string(h) + ".linear.bias", 0, 1, g);
    }
    const size_t act = (size_t)t->M * FILTERS;
    const int kmax = 9 * (t->np > FILTERS ? t->np : FILTERS);
    t->pstride = 2 * (FILTERS + 1 + t->nn + 1);
    do {
        if ((rc = dalloc(t, &t->P, t->total))) break;
        if ((rc = dalloc(t, &t->G, t->total))) break;
        if ((rc = dalloc(t, &t->M1, t->total))) break;
        if ((rc = dalloc(t, &t->M2, t->total))) break;
        if ((rc = dalloc(t, &t->group_dev, t->total / 1024))) break;
        if ((rc = dalloc(t, &t->states, (size_t)batch))) break;
        if ((rc = dalloc(t, &t->x0, (size_t)t->M * t->cin))) break;
        t->c.resize(t->layers);
        t->a.resize(t->layers);
        for (int l = 0; l < t->layers && !rc; l++) {
            if ((rc = dalloc(t, &t->c[l], act))) break;
            rc = dalloc(t, &t->a[l], act);
        }
        if (rc) break;
        if ((rc = dalloc(t, &t->stats, (size_t)t->layers * 2 * FILTERS))) break;
        if ((rc = dalloc(t, &t->partial, (size_t)SPLITS * FILTERS * 2))) break;
        if ((rc = dalloc(t, &t->mean_dy, (size_t)FILTERS))) break;
        if ((rc = dalloc(t, &t->mean_dyx, (size_t)FILTERS))) break;
        t->kmax = kmax;
        if ((rc = dalloc(t, &t->wmirror, (size_t)t->layers * kmax * FILTERS))) break;
        if ((rc = dalloc(t, &t->dA, act))) break;
        if ((rc = dalloc(t, &t->dB, act))) break;
        if ((rc = dalloc(t, &t->dC, act))) break;
        if ((rc = dalloc(t, &t->dC2, act))) break;
        {
            int cus = 0;
            if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, t->device) == hipSuccess && cus > 0) t->sk_groups = 2 * cus;
            if ((rc = dalloc(t, &t->sk_ws[0], (size_t)t->sk_groups * 2 * 4096))) break;
            if ((rc = dalloc(t, &t->sk_ws[1], (size_t)t->sk_groups * 2 * 4096))) break;
        }
        if ((rc = dalloc(t, &t->dskip, act))) break;
        if ((rc = dalloc(t, &t->pol, (size_t)t->M * t->np))) break;
        if ((rc = dalloc(t, &t->dpol, (size_t)t->M * t->np))) break;
        if ((rc = dalloc(t, &t->pre, (size_t)2 * t->M))) break;
        if ((rc = dalloc(t, &t->value, (size_t)batch))) break;
        if ((rc = dalloc(t, &t->ube, (size_t)batch))) break;
        if ((rc = dalloc(t, &t->tpol, (size_t)batch * t->pol_ch * t->nn))) break;
        if ((rc = dalloc(t, &t->mask, (size_t)batch * t->pol_ch * t->nn))) break;
        if ((rc = dalloc(t, &t->tv, (size_t)batch))) break;
        if ((rc = dalloc(t, &t->tu, (size_t)batch))) break;
        if ((rc = dalloc(t, &t->part, (size_t)batch * t->pstride))) break;
        if ((rc = dalloc(t, &t->loss_p, (size_t)batch))) break;
        if ((rc = dalloc(t, &t->loss_v, (size_t)batch))) break;
        if ((rc = dalloc(t, &t->loss_u, (size_t)batch))) break;
        if ((rc = dalloc(t, &t->losses, (size_t)4))) break;
    } while (0);
    if (!rc && (hipStreamCreate(&t->stream) != hipSuccess || hipStreamCreate(&t->stream2) != hipSuccess))
        rc = tz_fail(TZ_EDEVICE, "tz_trainer_create: stream");
    if (!rc && hipEventCreateWithFlags(&t->ev_mirror, hipEventDisableTiming) != hipSuccess) rc = tz_fail(TZ_EDEVICE, "tz_trainer_create: event");
    for (int i = 0; i < 2 && !rc; i++)
        if (hipEventCreateWithFlags(&t->ev_dc[i], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&t->ev_w[i], hipEventDisableTiming) != hipSuccess)
            rc = tz_fail(TZ_EDEVICE, "tz_trainer_create: event");
    if (!rc) {
        std::vector<uint8_t> groups(t->total / 1024, 0);
        for (const Param& p : t->params)
            for (size_t b = 0; b < p.slots / 1024; b++) groups[p.off / 1024 + b] = (uint8_t)p.group;
        if (hipMemcpy(t->group_dev, groups.data(), groups.size(), hipMemcpyHostToDevice) != hipSuccess)
            rc = tz_fail(TZ_EDEVICE, "tz_trainer_create: upload");
    }
    if (rc) {
        for (void* q : t->allocs) (void)hipFree(q);
        if (t->stream) (void)hipStreamDestroy(t->stream);
        if (t->stream2) (void)hipStreamDestroy(t->stream2);
        for (int i = 0; i < 2; i++) {
            if (t->ev_dc[i]) (void)hipEventDestroy(t->ev_dc[i]);
            if (t->ev_w[i]) (void)hipEventDestroy(t->ev_w[i]);
        }
        delete t;
        return rc;
    }
    *out = t;
    return TZ_OK;
}

int tz_trainer_destroy(tz_trainer* t) {
    if (!t) return TZ_OK;
    (void)hipSetDevice(t->device);
    (void)hipStreamSynchronize(t->stream);
    (void)hipStreamSynchronize(t->stream2);
    if (t->rnd.stream) {
        (void)hipStreamSynchronize(t->rnd.stream);
        (void)hipStreamDestroy(t->rnd.stream);
    }
    if (t->rnd.ev_x0) (void)hipEventDestroy(t->rnd.ev_x0);
    if (t->rnd.ev_done) (void)hipEventDestroy(t->rnd.ev_done);
    tz_rnd4l_destroy(t->rnd4);
    for (void* q : t->allocs) (void)hipFree(q);
    (void)hipStreamDestroy(t->stream);
    (void)hipStreamDestroy(t->stream2);
    for (int i = 0; i < 2; i++) {
        (void)hipEventDestroy(t->ev_dc[i]);
        (void)hipEventDestroy(t->ev_w[i]);
    }
    if (t->ev_mirror) (void)hipEventDestroy(t->ev_mirror);
    delete t;
    return TZ_OK;
}

// number of tensors the trainer owns, and the name / element count of tensor i (reference names, `.a.` / `.b.`)
int tz_trainer_shape(tz_trainer* t, int* board_n_out, int* batch_out, int* arch_out) {
    if (!t) return tz_fail(TZ_EINVAL, "tz_trainer_shape: null handle");
    if (board_n_out) *board_n_out = t->n;
    if (batch_out) *batch_out = t->batch;
    if (arch_out) *arch_out = t->arch;
    return TZ_OK;
}

int tz_trainer_tensor_count(tz_trainer* t) { return t ? (int)t->params.size() : 0; }

int tz_trainer_tensor_info(tz_trainer* t, int i, char* name_out, int name_cap, uint64_t* count_out) {
    if (!t || i < 0 || i >= (int)t->params.size() || !name_out || name_cap <= 0)
        return tz_fail(TZ_EINVAL, "tz_trainer_tensor_info: bad argument");
    const Param& p = t->params[i];
    if ((int)p.name.size() + 1 > name_cap) return tz_fail(TZ_EINVAL, "tz_trainer_tensor_info: name buffer too small");
    memcpy(name_out, p.name.c_str(), p.name.size() + 1);
    if (count_out) *count_out = p.count;
    return TZ_OK;
}

static float* arena_of(tz_trainer* t, int what) {
    return what == 0 ? t->P : what == 1 ? t->G : what == 2 ? t->M1 : what == 3 ? t->M2 : nullptr;
}

// what: 0 parameter, 1 gradient of the last step, 2 / 3 Adam first / second moment.  Data in the reference's layout.
int tz_trainer_set_tensor(tz_trainer* t, const char* name, int what, const float* data, uint64_t count) {
    if (!t || !name || !data) return tz_fail(TZ_EINVAL, "tz_trainer_set_tensor: null argument");
    if (t->rnd.on && rnd_index(name) >= 0) {   // the predictor's variables answer while its training is enabled
        Rnd& r = t->rnd;
        const int i = rnd_index(name);
        float* ra = what == 0 ? r.P : what == 1 ? r.G : what == 2 ? r.M1 : what == 3 ? r.M2 : nullptr;
        if (!ra) return tz_fail(TZ_EINVAL, std::string("tz_trainer_set_tensor: unknown tensor ") + name);
        if (count != rnd_count(i)) return tz_fail(TZ_EPARSE, std::string("tz_trainer_set_tensor: wrong size for ") + name);
        TZ_HIP(hipSetDevice(t->device));
        std::vector<float> host;
        rnd_pack(i, data, host, r.slots[i]);
        TZ_HIP(hipStreamSynchronize(t->stream));
        TZ_HIP(hipStreamSynchronize(r.stream));
        TZ_HIP(hipMemcpy(ra + r.off[i], host.data(), r.slots[i] * sizeof(float), hipMemcpyHostToDevice));
        return TZ_OK;
    }
    {
        size_t off, n;
        int kind, ci;
        if (rnd4_on(t) && tz_rnd4l_find(name, off, n, kind, ci)) {   // net4_rnd's predictor tower, while its training is enabled
            TZ_HIP(hipSetDevice(t->device));
            TZ_HIP(hipStreamSynchronize(t->stream));
            return tz_rnd4l_set(t->rnd4, name, what, data, count);
        }
    }
    size_t eoff = 0, ecount = 0;
    if (t->ens.armed && ens_find(name, eoff, ecount)) {   // the heads' variables answer while the trainer is armed
        Ens& e = t->ens;
        float* ea = what == 0 ? e.P : what == 1 ? e.G : what == 2 ? e.M1 : what == 3 ? e.M2 : nullptr;
        if (!ea) return tz_fail(TZ_EINVAL, std::string("tz_trainer_set_tensor: unknown tensor ") + name);
        if (count != ecount) return tz_fail(TZ_EPARSE, std::string("tz_trainer_set_tensor: wrong size for ") + name);
        TZ_HIP(hipSetDevice(t->device));
        TZ_HIP(hipStreamSynchronize(t->stream));
        TZ_HIP(hipMemcpy(ea + eoff, data, ecount * sizeof(float), hipMemcpyHostToDevice));
        return TZ_OK;
    }
    auto it = t->index.find(name);
    float* arena = arena_of(t, what);
    if (it == t->index.end() || !arena) return tz_fail(TZ_EINVAL, std::string("tz_trainer_set_tensor: unknown tensor ") + name);
    const Param& p = t->params[it->second];
    if (count != p.count) return tz_fail(TZ_EPARSE, std::string("tz_trainer_set_tensor: wrong size for ") + name);
    TZ_HIP(hipSetDevice(t->device));
    std::vector<float> host(p.slots, 0.f);
    if (p.kind == 1) {
        for (int co = 0; co < p.co; co++)
            for (int ci = 0; ci < p.ci; ci++)
                for (int tap = 0; tap < 9; tap++)
                    host[((size_t)tap * p.ci + ci) * p.ld + co] = data[((size_t)co * p.ci + ci) * 9 + tap];
    } else {
        memcpy(host.data(), data, count * sizeof(float));
    }
    TZ_HIP(hipStreamSynchronize(t->stream));
    TZ_HIP(hipMemcpy(arena + p.off, host.data(), p.slots * sizeof(float), hipMemcpyHostToDevice));
    return TZ_OK;
}

int tz_trainer_get_tensor(tz_trainer* t, const char* name, int what, float* out, uint64_t count) {
    if (!t || !name || !out) return tz_fail(TZ_EINVAL, "tz_trainer_get_tensor: null argument");
    if (t->rnd.on && rnd_index(name) >= 0) {
        Rnd& r = t->rnd;
        const int i = rnd_index(name);
        const float* ra = what == 0 ? r.P : what == 1 ? r.G : what == 2 ? r.M1 : what == 3 ? r.M2 : nullptr;
        if (!ra) return tz_fail(TZ_EINVAL, std::string("tz_trainer_get_tensor: unknown tensor ") + name);
        if (count != rnd_count(i)) return tz_fail(TZ_EPARSE, std::string("tz_trainer_get_tensor: wrong size for ") + name);
        TZ_HIP(hipSetDevice(t->device));
        std::vector<float> host(r.slots[i]);
        TZ_HIP(hipStreamSynchronize(t->stream));
        TZ_HIP(hipStreamSynchronize(r.stream));
        TZ_HIP(hipMemcpy(host.data(), ra + r.off[i], r.slots[i] * sizeof(float), hipMemcpyDeviceToHost));
        rnd_unpack(i, host, out);
        return TZ_OK;
    }
    {
        size_t off, n;
        int kind, ci;
        if (rnd4_on(t) && tz_rnd4l_find(name, off, n, kind, ci)) {
            TZ_HIP(hipSetDevice(t->device));
            TZ_HIP(hipStreamSynchronize(t->stream));
            return tz_rnd4l_get(t->rnd4, name, what, out, count);
        }
    }
    size_t eoff = 0, ecount = 0;
    if (t->ens.armed && ens_find(name, eoff, ecount)) {
        const Ens& e = t->ens;
        const float* ea = what == 0 ? e.P : what == 1 ? e.G : what == 2 ? e.M1 : what == 3 ? e.M2 : nullptr;
        if (!ea) return tz_fail(TZ_EINVAL, std::string("tz_trainer_get_tensor: unknown tensor ") + name);
        if (count != ecount) return tz_fail(TZ_EPARSE, std::string("tz_trainer_get_tensor: wrong size for ") + name);
        TZ_HIP(hipSetDevice(t->device));
        TZ_HIP(hipStreamSynchronize(t->stream));
        TZ_HIP(hipMemcpy(out, ea + eoff, ecount * sizeof(float), hipMemcpyDeviceToHost));
        return TZ_OK;
    }
    auto it = t->index.find(name);
    float* arena = arena_of(t, what);
    if (it == t->index.end() || !arena) return tz_fail(TZ_EINVAL, std::string("tz_trainer_get_tensor: unknown tensor ") + name);
    const Param& p = t->params[it->second];
    if (count != p.count) return tz_fail(TZ_EPARSE, std::string("tz_trainer_get_tensor: wrong size for ") + name);
    TZ_HIP(hipSetDevice(t->device));
    std::vector<float> host(p.slots);
    TZ_HIP(hipStreamSynchronize(t->stream));
    TZ_HIP(hipMemcpy(host.data(), arena + p.off, p.slots * sizeof(float), hipMemcpyDeviceToHost));
    if (p.kind == 1) {
        for (int co = 0; co < p.co; co++)
            for (int ci = 0; ci < p.ci; ci++)
                for (int tap = 0; tap < 9; tap++)
                    out[((size_t)co * p.ci + ci) * 9 + tap] = host[((size_t)tap * p.ci + ci) * p.ld + co];
    } else {
        memcpy(out, host.data(), count * sizeof(float));
    }
    return TZ_OK;
}

// shape of a variable in the reference's VarStore
static std::vector<uint32_t> param_dims(const tz_trainer* t, const Param& p) {
    auto ends = [&](const char* s) { const size_t n = strlen(s); return p.name.size() >= n && !p.name.compare(p.name.size() - n, n, s); };
    if (p.kind == 1) return {(uint32_t)p.co, (uint32_t)p.ci, 3u, 3u};
    if (ends("value.conv2d.weight") || ends("ube.conv2d.weight")) return {1u, (uint32_t)p.count, 1u, 1u};
    if (ends(".linear.weight")) return {1u, (uint32_t)t->nn};
    return {(uint32_t)p.count};
}

// The trainer's VarStore as a host store (current parameters and buffers + the carried extras)
int tz_trainer_snapshot(tz_trainer* t, TensorStore& out) {
    if (t->rnd.on) {
        int rc = rnd_download(t);
        if (rc) return rc;
    }
    if (t->ens.armed) {
        int rc = ens_download(t);
        if (rc) return rc;
    }
    if (rnd4_on(t)) {
        TZ_HIP(hipSetDevice(t->device));
        TZ_HIP(hipStreamSynchronize(t->stream));
        int rc = tz_rnd4l_download(t->rnd4, t->extra);
        if (rc) return rc;
    }
    out = t->extra;
    for (const Param& p : t->params) {
        HostTensor h;
        h.dims = param_dims(t, p);
        h.data.resize(p.count);
        int rc = tz_trainer_get_tensor(t, p.name.c_str(), 0, h.data.data(), p.count);
        if (rc) return rc;
        out[p.name] = std::move(h);
    }
    return TZ_OK;
}

static int trainer_apply_store(tz_trainer* t, const TensorStore& st) {
    for (const Param& p : t->params) {
        auto it = st.find(p.name);
        if (it == st.end()) return tz_fail(TZ_EPARSE, "trainer: the model has no variable " + p.name);
        if (it->second.data.size() != p.count) return tz_fail(TZ_EPARSE, "trainer: wrong size of variable " + p.name);
    }
    for (const Param& p : t->params) {
        int rc = tz_trainer_set_tensor(t, p.name.c_str(), 0, st.at(p.name).data.data(), p.count);
        if (rc) return rc;
    }
    t->extra.clear();
    for (auto& kv : st)
        if (!t->index.count(kv.first)) t->extra[kv.first] = kv.second;
    if (t->ens.armed) {   // the loaded model's heads replace the device's (moments stay, as for the other parameters)
        if (!ens_variables_present(t)) {
            t->ens.armed = false;
            return tz_fail(TZ_ESTATE, "trainer: the loaded model holds no ensemble heads; the trainer is disarmed");
        }
        int rc = ens_upload(t);
        if (rc) return rc;
    }
    if (rnd4_on(t)) {   // the loaded model's towers replace the device's (moments stay, as for the other parameters)
        if (!tz_rnd4l_present(t->extra)) {
            t->rnd4->on = false;
            return tz_fail(TZ_ESTATE, "trainer: the loaded model holds no RND towers; their training is switched off");
        }
        TZ_HIP(hipStreamSynchronize(t->stream));
        int rc = tz_rnd4l_upload(t->rnd4, t->extra);
        if (rc) return rc;
    }
    if (t->rnd.on) {   // the loaded model's RND nets replace the device's (moments stay, as for the other parameters)
        if (!rnd_variables_present(t)) {
            t->rnd.on = false;
            return tz_fail(TZ_ESTATE, "trainer: the loaded model holds no RND variables; RND training is switched off");
        }
        return rnd_upload(t);
    }
    return TZ_OK;
}

// Network::load / Network::save on the trainer's VarStore (learn/src/main.rs:107-120, 247-266): LibTorch archive or .tzw
int tz_trainer_load(tz_trainer* t, const char* path) {
    if (!t || !path) return tz_fail(TZ_EINVAL, "tz_trainer_load: null argument");
    TensorStore st;
    int rc = weights_read_file(path, st);
    if (rc) return rc;
    return trainer_apply_store(t, st);
}

// the same from a .tzw container in memory (how the Python wrapper hands over a dict of tensors, extras included)
int tz_trainer_load_weights_mem(tz_trainer* t, const void* data, size_t bytes) {
    if (!t || !data) return tz_fail(TZ_EINVAL, "tz_trainer_load_weights_mem: null argument");
    TensorStore st;
    int rc = tzw_parse(static_cast<const unsigned char*>(data), bytes, st);
    if (rc) return rc;
    return trainer_apply_store(t, st);
}

// the carried variables alone as a .tzw container: out = NULL (or cap too small) asks for the size only
int tz_trainer_get_extras(tz_trainer* t, void* out, uint64_t cap, uint64_t* bytes_out) {
    if (!t) return tz_fail(TZ_EINVAL, "tz_trainer_get_extras: null handle");
    if (t->rnd.on) {
        int rc = rnd_download(t);
        if (rc) return rc;
    }
    if (t->ens.armed) {
        int rc = ens_download(t);
        if (rc) return rc;
    }
    if (rnd4_on(t)) {
        TZ_HIP(hipSetDevice(t->device));
        TZ_HIP(hipStreamSynchronize(t->stream));
        int rc = tz_rnd4l_download(t->rnd4, t->extra);
        if (rc) return rc;
    }
    std::vector<unsigned char> blob;
    tzw_dump(t->extra, blob);
    if (bytes_out) *bytes_out = blob.size();
    if (out && cap >= blob.size()) memcpy(out, blob.data(), blob.size());
    return TZ_OK;
}

int tz_trainer_save(tz_trainer* t, const char* path) {
    if (!t || !path) return tz_fail(TZ_EINVAL, "tz_trainer_save: null argument");
    TensorStore st;
    int rc = tz_trainer_snapshot(t, st);
    if (rc) return rc;
    return weights_write_file(path, st);
}

// the variables of a network (Net::new / a loaded model) become the trainer's, and back without a file
int tz_trainer_from_net(tz_trainer* t, tz_net* net) {
    if (!t || !net) return tz_fail(TZ_EINVAL, "tz_trainer_from_net: null argument");
    if (!net->loaded) return tz_fail(TZ_ESTATE, "tz_trainer_from_net: the network has no weights");
    return trainer_apply_store(t, net->store);
}

int tz_trainer_to_net(tz_trainer* t, tz_net* net) {
    if (!t || !net) return tz_fail(TZ_EINVAL, "tz_trainer_to_net: null argument");
    TensorStore st;
    int rc = tz_trainer_snapshot(t, st);
    if (rc) return rc;
    std::vector<unsigned char> blob;
    tzw_dump(st, blob);
    return tz_net_load_weights_mem(net, blob.data(), blob.size());
}

// compute_loss_and_take_step (learn/src/main.rs:376-423) on one batch:
//   states[batch]; target_policy[batch][policy_size] (policy_tensor); mask[batch][policy_size], 1 = not a legal move
//   (move_mask); target_value[batch]; target_ube[batch] = variance targets (the log / clamp of :360-363 is applied here).
//   losses_out[3] = policy, value, ube.  apply_step = 0 computes losses and gradients only.
int tz_trainer_step(tz_trainer* t, const tz_state* states, const float* target_policy, const uint8_t* mask,
                    const float* target_value, const float* target_ube, int train_ube, int apply_step, float* losses_out) {
    if (!t || !states || !target_policy || !mask || !target_value || !target_ube)
        return tz_fail(TZ_EINVAL, "tz_trainer_step: null argument");
    TZ_HIP(hipSetDevice(t->device));
    const size_t out = (size_t)t->pol_ch * t->nn;
    TZ_HIP(hipMemcpyAsync(t->states, states, sizeof(tz_state) * t->batch, hipMemcpyHostToDevice, t->stream));
    TZ_HIP(hipMemcpyAsync(t->tpol, target_policy, sizeof(float) * t->batch * out, hipMemcpyHostToDevice, t->stream));
    TZ_HIP(hipMemcpyAsync(t->mask, mask, (size_t)t->batch * out, hipMemcpyHostToDevice, t->stream));
    TZ_HIP(hipMemcpyAsync(t->tv, target_value, sizeof(float) * t->batch, hipMemcpyHostToDevice, t->stream));
    TZ_HIP(hipMemcpyAsync(t->tu, target_ube, sizeof(float) * t->batch, hipMemcpyHostToDevice, t->stream));
    int rc;
    // (forward + backward captured as one HIP graph per train_ube was measured and not kept: 9.27 against 7.90 ms per step — the
    // graph's two branches do not overlap the way the two streams do)
    if ((rc = mirror_all(t))) return rc;
    if ((rc = forward(t))) return rc;
    if (t->rnd.on && (rc = rnd_chain(t, apply_step))) return rc;
    if (rnd4_on(t) && (rc = rnd4_chain(t, apply_step))) return rc;
    if ((rc = backward(t, train_ube))) return rc;
    if (t->rnd.on) TZ_HIP(hipStreamWaitEvent(t->stream, t->rnd.ev_done, 0));
    if (rnd4_on(t)) TZ_HIP(hipStreamWaitEvent(t->stream, t->rnd4->ev_done, 0));
    if (t->ens.armed && (rc = ens_chain(t, apply_step))) return rc;
    if (apply_step) {
        t->t_main++;
        if (train_ube) t->t_ube++;
        adam_kernel<<<(unsigned)(t->total / 1024), 256, 0, t->stream>>>(t->P, t->G, t->M1, t->M2, t->group_dev, t->lr,
                                                                        t->t_main, train_ube ? t->t_ube : 0, 0);
        if ((rc = launch_check("adam"))) return rc;
    }
    float losses[4] = {0, 0, 0, 0}, loss_ens = 0.f;
    TZ_HIP(hipMemcpyAsync(losses, t->losses, sizeof(float) * 3, hipMemcpyDeviceToHost, t->stream));
    if (t->ens.armed) TZ_HIP(hipMemcpyAsync(&loss_ens, t->ens.loss, sizeof(float), hipMemcpyDeviceToHost, t->stream));
    if (t->rnd.on) TZ_HIP(hipMemcpyAsync(&losses[3], t->rnd.loss, sizeof(float), hipMemcpyDeviceToHost, t->stream));
    if (rnd4_on(t)) TZ_HIP(hipMemcpyAsync(&losses[3], t->rnd4->loss, sizeof(float), hipMemcpyDeviceToHost, t->stream));
    TZ_HIP(hipStreamSynchronize(t->stream));
    if (t->rnd.on) {
        t->rnd.last_loss = losses[3];
        t->rnd.have_last = true;
    }
    if (t->ens.armed) {
        t->ens.last_loss = loss_ens;
        t->ens.have_last = true;
    }
    if (rnd4_on(t)) {
        t->rnd4->last_loss = losses[3];
        t->rnd4->have_last = true;
    }
    if (losses_out) memcpy(losses_out, losses, sizeof(float) * 3);
    if (!(losses[0] == losses[0]) || !(losses[1] == losses[1]) || !(losses[2] == losses[2]))
        return tz_fail(TZ_ENUMERIC, "tz_trainer_step: a loss is NaN");
    if ((t->rnd.on || rnd4_on(t)) && !(losses[3] == losses[3])) return tz_fail(TZ_ENUMERIC, "tz_trainer_step: loss_rnd is NaN");
    if (t->ens.armed && !(loss_ens == loss_ens)) return tz_fail(TZ_ENUMERIC, "tz_trainer_step: loss_ensemble is NaN");
    return TZ_OK;
}

// network outputs of the last step's forward pass (training mode): policy [batch][policy_size] in the reference's
// c*nn + px order, value [batch] (after tanh), ube [batch] (log variance)
int tz_trainer_outputs(tz_trainer* t, float* policy_out, float* value_out, float* ube_out) {
    if (!t) return tz_fail(TZ_EINVAL, "tz_trainer_outputs: null trainer");
    TZ_HIP(hipSetDevice(t->device));
    TZ_HIP(hipStreamSynchronize(t->stream));
    if (policy_out) {
        std::vector<float> host((size_t)t->M * t->np);
        TZ_HIP(hipMemcpy(host.data(), t->pol, host.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int b = 0; b < t->batch; b++)
            for (int c = 0; c < t->pol_ch; c++)
                for (int px = 0; px < t->nn; px++)
                    policy_out[((size_t)b * t->pol_ch + c) * t->nn + px] = host[((size_t)b * t->nn + px) * t->np + c];
    }
    if (value_out) TZ_HIP(hipMemcpy(value_out, t->value, sizeof(float) * t->batch, hipMemcpyDeviceToHost));
    if (ube_out) TZ_HIP(hipMemcpy(ube_out, t->ube, sizeof(float) * t->batch, hipMemcpyDeviceToHost));
    return TZ_OK;
}

int tz_trainer_activation(tz_trainer* t, int layer, float* out, uint64_t cap) {
    if (!t || !out) return tz_fail(TZ_EINVAL, "tz_trainer_activation: null argument");
    if (layer < 0 || layer >= t->layers) return tz_fail(TZ_EINVAL, "tz_trainer_activation: no such trunk layer");
    const size_t real = (size_t)t->batch * t->nn * FILTERS;
    if (cap < real) return tz_fail(TZ_EINVAL, "tz_trainer_activation: the buffer holds fewer than batch * n * n * 256 values");
    TZ_HIP(hipSetDevice(t->device));
    TZ_HIP(hipStreamSynchronize(t->stream));
    TZ_HIP(hipMemcpy(out, t->a[layer], real * sizeof(float), hipMemcpyDeviceToHost));
    return TZ_OK;
}

// ---- training net4_ensemble's heads (eee/src/ensemble.rs:318-351) ----
int tz_trainer_set_ensemble_targets(tz_trainer* t, const float* targets) {
    if (!t) return tz_fail(TZ_EINVAL, "tz_trainer_set_ensemble_targets: null handle");
    if (t->arch != TZ_ARCH_NET4_ENSEMBLE) return tz_fail(TZ_EINVAL, "tz_trainer_set_ensemble_targets: only net4_ensemble has ensemble heads");
    TZ_HIP(hipSetDevice(t->device));
    int rc;
    if (!targets) {
        if (t->ens.armed && (rc = ens_download(t))) return rc;   // the trained heads stay with the carried variables
        t->ens.armed = false;
        return TZ_OK;
    }
    if (!t->ens.armed) {
        if (!ens_variables_present(t)) return tz_fail(TZ_ESTATE, "tz_trainer_set_ensemble_targets: the loaded variables hold no `ensemble head i.*`");
        if ((rc = ens_allocate(t))) return rc;
        if ((rc = ens_upload(t))) return rc;
        t->ens.armed = true;
    }
    TZ_HIP(hipStreamSynchronize(t->stream));
    TZ_HIP(hipMemcpy(t->ens.targets, targets, sizeof(float) * t->batch * ENS, hipMemcpyHostToDevice));
    return TZ_OK;
}

int tz_trainer_ensemble_last(tz_trainer* t, float* loss_out, float* values_out) {
    if (!t) return tz_fail(TZ_EINVAL, "tz_trainer_ensemble_last: null handle");
    if (!t->ens.allocated || !t->ens.have_last) return tz_fail(TZ_ESTATE, "tz_trainer_ensemble_last: no armed step yet");
    TZ_HIP(hipSetDevice(t->device));
    TZ_HIP(hipStreamSynchronize(t->stream));
    if (loss_out) *loss_out = t->ens.last_loss;
    if (values_out) TZ_HIP(hipMemcpy(values_out, t->ens.values, sizeof(float) * t->batch * ENS, hipMemcpyDeviceToHost));
    return TZ_OK;
}

// ---- RND training (net5.rs:193-218; learn/src/main.rs:404-405, 415-416; learn/src/rnd_normalization.rs:74-78) ----
int tz_trainer_rnd_enable(tz_trainer* t, int on) {
    if (!t) return tz_fail(TZ_EINVAL, "tz_trainer_rnd_enable: null handle");
    if (t->arch != TZ_ARCH_NET5) return tz_fail(TZ_EINVAL, "tz_trainer_rnd_enable: only net5 has RND networks");
    TZ_HIP(hipSetDevice(t->device));
    int rc;
    if (!on) {
        if (t->rnd.on && (rc = rnd_download(t))) return rc;   // the trained predictor stays with the carried variables
        t->rnd.on = false;
        return TZ_OK;
    }
    if (t->rnd.on) return TZ_OK;
    if (!rnd_variables_present(t))
        return tz_fail(TZ_ESTATE, "tz_trainer_rnd_enable: the loaded variables hold no rnd_learning.* / rnd_target.* / min / max");
    if ((rc = rnd_allocate(t))) return rc;
    if ((rc = rnd_upload(t))) return rc;
    t->rnd.on = true;
    return TZ_OK;
}

int tz_trainer_rnd_last(tz_trainer* t, float* loss_out, float* raw_out) {
    if (!t) return tz_fail(TZ_EINVAL, "tz_trainer_rnd_last: null handle");
    if (!t->rnd.allocated || !t->rnd.have_last) return tz_fail(TZ_ESTATE, "tz_trainer_rnd_last: no step with RND training yet");
    TZ_HIP(hipSetDevice(t->device));
    TZ_HIP(hipStreamSynchronize(t->stream));
    if (loss_out) *loss_out = t->rnd.last_loss;
    if (raw_out) TZ_HIP(hipMemcpy(raw_out, t->rnd.raw, sizeof(float) * t->batch, hipMemcpyDeviceToHost));
    return TZ_OK;
}

int tz_trainer_rnd_activation(tz_trainer* t, int which, int layer, float* out, uint64_t out_cap) {
    if (!t || !out) return tz_fail(TZ_EINVAL, "tz_trainer_rnd_activation: null argument");
    if (which < 0 || which > 1 || layer < 0 || layer > 2) return tz_fail(TZ_EINVAL, "tz_trainer_rnd_activation: no such network or layer");
    if (!t->rnd.allocated) return tz_fail(TZ_ESTATE, "tz_trainer_rnd_activation: RND training was never enabled");
    const size_t real = (size_t)t->batch * (layer == 2 ? RND_OUT : RND_HID);
    if (out_cap < real) return tz_fail(TZ_EINVAL, "tz_trainer_rnd_activation: the buffer is too small");
    TZ_HIP(hipSetDevice(t->device));
    TZ_HIP(hipStreamSynchronize(t->stream));
    TZ_HIP(hipStreamSynchronize(t->rnd.stream));
    TZ_HIP(hipMemcpy(out, layer == 2 ? t->rnd.out[which] : t->rnd.h[which][layer], real * sizeof(float), hipMemcpyDeviceToHost));
    return TZ_OK;
}

int tz_trainer_rnd_calibrate(tz_trainer* t, const tz_state* early, int n_early, const tz_state* late, int n_late, int apply,
                             float* min_out, float* max_out) {
    if (!t || !early || !late || n_early < 1 || n_late < 1) return tz_fail(TZ_EINVAL, "tz_trainer_rnd_calibrate: bad argument");
    if (!t->rnd.on) return tz_fail(TZ_ESTATE, "tz_trainer_rnd_calibrate: RND training is not enabled");
    Rnd& r = t->rnd;
    TZ_HIP(hipSetDevice(t->device));
    TZ_HIP(hipStreamSynchronize(t->stream));
    const int B = t->batch;
    std::vector<tz_state> chunk(B);
    float found[2] = {INFINITY, -INFINITY};   // min over early, max over late
    for (int set = 0; set < 2; set++) {
        const tz_state* states = set ? late : early;
        const int count = set ? n_late : n_early;
        for (int c = 0; c < count; c += B) {
            const int cnt = std::min(B, count - c);
            for (int i = 0; i < B; i++) chunk[i] = states[c + (i < cnt ? i : 0)];   // the rows past cnt repeat one and are not read back
            TZ_HIP(hipMemcpyAsync(t->states, chunk.data(), sizeof(tz_state) * B, hipMemcpyHostToDevice, r.stream));
            int rc;
            if ((rc = tz_nn_encode_planes(t->n, t->cin, t->states, B, t->x0, r.stream))) return rc;
            if ((rc = rnd_forward(t, r.stream))) return rc;
            rnd_distance_kernel<<<B, 256, 0, r.stream>>>(r.out[0], r.out[1], B, r.raw_cal, nullptr);
            rnd_minmax_kernel<<<1, 256, 0, r.stream>>>(r.raw_cal, cnt, r.minmax);
            if ((rc = launch_check("rnd calibrate"))) return rc;
            float mm[2];
            TZ_HIP(hipMemcpyAsync(mm, r.minmax, sizeof mm, hipMemcpyDeviceToHost, r.stream));
            TZ_HIP(hipStreamSynchronize(r.stream));
            if (set == 0) found[0] = fminf(found[0], mm[0]);
            else found[1] = fmaxf(found[1], mm[1]);
        }
    }
    if (min_out) *min_out = found[0];
    if (max_out) *max_out = found[1];
    if (!(found[1] > found[0])) return tz_fail(TZ_ESTATE, "tz_trainer_rnd_calibrate: max is not above min; the variables are left alone");
    if (apply) {
        t->extra["min"].data[0] = found[0];
        t->extra["max"].data[0] = found[1];
    }
    return TZ_OK;
}

// ---- training net4_rnd's predictor tower (net4_rnd.rs:126-166, 210-223; learn/src/main.rs:404-405; learn/src/rnd_normalization.rs:74-78) ----
int tz_trainer_rnd4_enable(tz_trainer* t, int on) {
    if (!t) return tz_fail(TZ_EINVAL, "tz_trainer_rnd4_enable: null handle");
    if (t->arch != TZ_ARCH_NET4_RND) return tz_fail(TZ_EINVAL, "tz_trainer_rnd4_enable: only net4_rnd has RND towers");
    TZ_HIP(hipSetDevice(t->device));
    TZ_HIP(hipStreamSynchronize(t->stream));
    int rc;
    if (!on) {
        if (rnd4_on(t) && (rc = tz_rnd4l_download(t->rnd4, t->extra))) return rc;   // the trained predictor stays with the carried variables
        if (t->rnd4) t->rnd4->on = false;
        return TZ_OK;
    }
    if (rnd4_on(t)) return TZ_OK;
    if (!tz_rnd4l_present(t->extra))
        return tz_fail(TZ_ESTATE, "tz_trainer_rnd4_enable: the loaded variables hold no rnd_predictor.* / rnd_target.* / min / max");
    if (!t->rnd4 && (rc = tz_rnd4l_create(t->batch, t->device, &t->rnd4))) return rc;
    if ((rc = tz_rnd4l_upload(t->rnd4, t->extra))) return rc;
    t->rnd4->on = true;
    return TZ_OK;
}

int tz_trainer_rnd4_last(tz_trainer* t, float* loss_out, float* raw_out) {
    if (!t) return tz_fail(TZ_EINVAL, "tz_trainer_rnd4_last: null handle");
    if (!t->rnd4 || !t->rnd4->have_last) return tz_fail(TZ_ESTATE, "tz_trainer_rnd4_last: no step with the predictor's training yet");
    TZ_HIP(hipSetDevice(t->device));
    TZ_HIP(hipStreamSynchronize(t->stream));
    TZ_HIP(hipStreamSynchronize(t->rnd4->stream));
    if (loss_out) *loss_out = t->rnd4->last_loss;
    if (raw_out) TZ_HIP(hipMemcpy(raw_out, t->rnd4->raw, sizeof(float) * t->batch, hipMemcpyDeviceToHost));
    return TZ_OK;
}

int tz_trainer_rnd4_activation(tz_trainer* t, int which, int layer, float* out, uint64_t out_cap) {
    if (!t || !out) return tz_fail(TZ_EINVAL, "tz_trainer_rnd4_activation: null argument");
    if (!t->rnd4) return tz_fail(TZ_ESTATE, "tz_trainer_rnd4_activation: the predictor's training was never enabled");
    TZ_HIP(hipSetDevice(t->device));
    TZ_HIP(hipStreamSynchronize(t->stream));
    return tz_rnd4l_activation(t->rnd4, which, layer, out, out_cap);
}

int tz_trainer_rnd4_calibrate(tz_trainer* t, const tz_state* early, int n_early, const tz_state* late, int n_late, int apply,
                              float* min_out, float* max_out) {
    if (!t || !early || !late || n_early < 1 || n_late < 1) return tz_fail(TZ_EINVAL, "tz_trainer_rnd4_calibrate: bad argument");
    if (!rnd4_on(t)) return tz_fail(TZ_ESTATE, "tz_trainer_rnd4_calibrate: the predictor's training is not enabled");
    TZ_HIP(hipSetDevice(t->device));
    TZ_HIP(hipStreamSynchronize(t->stream));
    float found[2];
    int rc;
    if ((rc = tz_rnd4l_calibrate(t->rnd4, early, n_early, late, n_late, found))) return rc;
    if (min_out) *min_out = found[0];
    if (max_out) *max_out = found[1];
    if (!(found[1] > found[0])) return tz_fail(TZ_ESTATE, "tz_trainer_rnd4_calibrate: max is not above min; the variables are left alone");
    if (apply) {
        t->extra["min"].data[0] = found[0];
        t->extra["max"].data[0] = found[1];
    }
    return TZ_OK;
}

}  // extern "C"
