// tz_learn_rnd4.hip — the distillation step of TZ_ARCH_NET4_RND's predictor tower (net4_rnd.rs:126-166, 210-223; residual.rs:8-63;
// learn/src/main.rs:404-405; eee/src/rnd.rs), fp32 throughout like the trainer.
//
//   forward    LayerNorm([28,4,4]) of the step's planes for both towers; the predictor in training mode (BatchNorm with the batch's mean
//              and biased variance, running statistics tracked with momentum 0.1 and the unbiased variance), the target in eval mode
//   loss       raw[b] = sum_512 (predictor - target)^2, loss = mean_b raw[b], dY = 2 (predictor - target) / batch
//   backward   through the predictor only: BatchNorm with batch statistics, ReLU masks from the stored activation, the residual
//              branches, data gradients against the transposed weights, weight gradients, LayerNorm's affine
//
// A layer is [batch * 16 rows] x [K = 9 taps * 32 channels] x [32 columns] (the first layer's channels 28..31 are zero), far from the
// trunk's 64x64 tiles: one wave owns a board (the 16 rows of v_mfma_f32_16x16x4_f32) and both 16-column tiles; a tap that leaves the
// board reads a zero row.  Activations are [row = board * 16 + square][32 channels].
//
// Every sum that crosses workgroups (batch statistics, BatchNorm's backward sums, weight gradients, LayerNorm's gradients, the loss) is
// written as per-workgroup partials and added by the consumer in partial order, in double: no atomics, the same bits every run.  One
// launch per dependent stage on a stream of its own beside the trunk; it reads the step's planes and nothing else of the trunk's.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "tz_learn_rnd4.h"

namespace {

constexpr int L = R4_LAYERS, CH = R4_CH, NN = R4_NN, GB = R4L_GROUP, WB = R4L_WBOARDS, WSZ = R4L_WSZ;
constexpr int PITCH = 36;             // LDS row of 32 channels, padded
constexpr float EPS = 1e-5f;          // tch LayerNormConfig / BatchNormConfig::default
constexpr float MOMENTUM = 0.1f;      // tch BatchNormConfig::default

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int tap_row(int square, int tap) {   // the source square of a tap, 16 (the zero row) off the board
    const int y = (square >> 2) + tap / 3 - 1, x = (square & 3) + tap % 3 - 1;
    return (y >= 0 && y < 4 && x >= 0 && x < 4) ? y * 4 + x : NN;
}

// a board's 16 x 32 floats into the wave's LDS image, and the zero row
__device__ __forceinline__ void load_board(float (*img)[PITCH], const float* __restrict__ src, int lane) {
#pragma unroll
    for (int j = 0; j < 2; j++) {
        const int i = lane * 4 + 256 * j;
        const float4 v = *reinterpret_cast<const float4*>(src + i);
        float* d = &img[i >> 5][i & 31];
        d[0] = v.x;
        d[1] = v.y;
        d[2] = v.z;
        d[3] = v.w;
    }
    if (lane < CH) img[NN][lane] = 0.f;
}

// LayerNorm over a position's 448 planes (population variance, two passes): xhat [batch][plane * 16 + square] and both towers' affine
// outputs [row][32].  One wave per board: lane holds elements lane + 64 k, sums its seven in order, then an xor butterfly.
__global__ __launch_bounds__(64) void r4l_ln_fwd_kernel(const float* __restrict__ x0, const float* __restrict__ P, const float* __restrict__ TP,
                                                       float* __restrict__ xhat, float* __restrict__ out_p, float* __restrict__ out_t) {
    const int b = blockIdx.x, lane = threadIdx.x;
    float x[7], sum = 0.f;
#pragma unroll
    for (int k = 0; k < 7; k++) {
        const int e = lane + 64 * k;
        x[k] = x0[((size_t)b * NN + (e & 15)) * R4_CIN + (e >> 4)];
        sum += x[k];
    }
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
    const float mean = sum / (float)R4_IN;
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < 7; k++) {
        x[k] -= mean;
        sq += x[k] * x[k];
    }
    for (int d = 32; d >= 1; d >>= 1) sq += __shfl_xor(sq, d);
    const float rstd = 1.0f / sqrtf(sq / (float)R4_IN + EPS);
#pragma unroll
    for (int k = 0; k < 7; k++) {
        const int e = lane + 64 * k;
        const float xh = x[k] * rstd;
        const size_t o = ((size_t)b * NN + (e & 15)) * CH + (e >> 4);
        xhat[(size_t)b * R4_IN + e] = xh;
        out_p[o] = xh * P[R4L_LNW + e] + P[R4L_LNB + e];
        out_t[o] = xh * TP[R4L_LNW + e] + TP[R4L_LNB + e];
    }
    const size_t z = ((size_t)b * NN + (lane & 15)) * CH + R4_CIN + (lane >> 4);
    out_p[z] = 0.f;
    out_t[z] = 0.f;
}

// conv 3x3 of GB boards, one per wave: c = im2col(in) x W, W [tap][ci][co].
//   EVAL = false (predictor): writes c and the workgroup's per-channel sum and sum of squares, part [workgroup][2][32]
//   EVAL = true  (target): a = (c - running_mean) / sqrt(running_var + eps) * weight + bias (+ skip), ReLU where `relu`
template <bool EVAL>
__global__ __launch_bounds__(256) void r4l_conv_fwd_kernel(const float* __restrict__ in, const float* __restrict__ W, float* __restrict__ out,
                                                          double* __restrict__ part, const float* __restrict__ gamma,
                                                          const float* __restrict__ running, const float* __restrict__ skip, int relu) {
    __shared__ float img[GB][NN + 1][PITCH];
    __shared__ double red[GB][2 * CH];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, col = lane & 15, q = lane >> 4;
    const size_t board = (size_t)blockIdx.x * GB + wave;
    load_board(img[wave], in + board * NN * CH, lane);
    __syncthreads();
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int tap = 0; tap < 9; tap++) {
        const float* arow = img[wave][tap_row(col, tap)];
        const float* wt = W + (size_t)tap * CH * CH;
#pragma unroll
        for (int kc = 0; kc < CH / 4; kc++) {
            const float av = arow[kc * 4 + q];
            const float* wr = wt + (kc * 4 + q) * CH;
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wr[col], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, wr[16 + col], acc[1], 0, 0, 0);
        }
    }
    // C/D: column = lane & 15, rows 4 (lane >> 4) + i
    float* o = out + (board * NN + q * 4) * CH;
    if (EVAL) {
#pragma unroll
        for (int ct = 0; ct < 2; ct++) {
            const int ch = ct * 16 + col;
            const float mean = running[ch], inv = 1.0f / sqrtf(running[CH + ch] + EPS), g = gamma[ch], bb = gamma[CH + ch];
#pragma unroll
            for (int i = 0; i < 4; i++) {
                float v = g * (acc[ct][i] - mean) * inv + bb;
                if (skip) v += skip[(board * NN + q * 4 + i) * CH + ch];
                o[i * CH + ch] = relu ? fmaxf(v, 0.f) : v;
            }
        }
        return;
    }
#pragma unroll
    for (int ct = 0; ct < 2; ct++) {
        double s = 0.0, s2 = 0.0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const float v = acc[ct][i];
            o[i * CH + ct * 16 + col] = v;
            s += (double)v;
            s2 += (double)v * (double)v;
        }
        s += __shfl_xor(s, 16);
        s2 += __shfl_xor(s2, 16);
        s += __shfl_xor(s, 32);
        s2 += __shfl_xor(s2, 32);
        if (q == 0) {
            red[wave][ct * 16 + col] = s;
            red[wave][CH + ct * 16 + col] = s2;
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * CH) {
        double s = 0.0;
        for (int w = 0; w < GB; w++) s += red[w][threadIdx.x];
        part[(size_t)blockIdx.x * 2 * CH + threadIdx.x] = s;
    }
}

// the partials of every workgroup in workgroup order, thread (kind, channel) = tid < 64
__device__ __forceinline__ void sum_partials(const double* __restrict__ part, int nparts, double* tot, int tid) {
    if (tid < 2 * CH) {
        double s = 0.0;
        for (int p = 0; p < nparts; p++) s += part[(size_t)p * 2 * CH + tid];
        tot[tid] = s;
    }
    __syncthreads();
}

// batch statistics (every workgroup adds the same partials in the same order), a = gamma * (c - mean) * invstd + beta (+ skip), ReLU
// where `relu`; workgroup 0 keeps mean / invstd for the backward and, with `track`, moves the running statistics (torch: the biased
// variance normalises, the unbiased one is tracked)
__global__ __launch_bounds__(256) void r4l_bn_act_kernel(const float* __restrict__ c, const double* __restrict__ part, int nparts, int rows,
                                                        const float* __restrict__ gamma, const float* __restrict__ skip, int relu,
                                                        float* __restrict__ a, float* __restrict__ stats, float* __restrict__ running,
                                                        int track) {
    __shared__ double tot[2 * CH];
    __shared__ float ms[2 * CH];
    const int tid = threadIdx.x;
    sum_partials(part, nparts, tot, tid);
    if (tid < CH) {
        const double mu = tot[tid] / rows;
        double var = tot[CH + tid] / rows - mu * mu;
        if (var < 0.0) var = 0.0;
        ms[tid] = (float)mu;
        ms[CH + tid] = (float)(1.0 / sqrt(var + (double)EPS));
        if (blockIdx.x == 0) {
            stats[tid] = ms[tid];
            stats[CH + tid] = ms[CH + tid];
            if (track) {
                running[tid] = (1.f - MOMENTUM) * running[tid] + MOMENTUM * (float)mu;
                running[CH + tid] = (1.f - MOMENTUM) * running[CH + tid] + MOMENTUM * (float)(var * rows / (rows - 1));
            }
        }
    }
    __syncthreads();
    const int ch = tid & 31;
    const float mean = ms[ch], inv = ms[CH + ch], g = gamma[ch], bb = gamma[CH + ch];
    const size_t i0 = ((size_t)blockIdx.x * GB * NN + (tid >> 5) * 8) * CH + ch;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const size_t i = i0 + (size_t)r * CH;
        float v = g * (c[i] - mean) * inv + bb;
        if (skip) v += skip[i];
        a[i] = relu ? fmaxf(v, 0.f) : v;
    }
}

// raw[b] = sum_512 (p - t)^2 (each lane its 8 in order, then the butterfly), dY = 2 (p - t) / batch
__global__ __launch_bounds__(64) void r4l_distance_kernel(const float* __restrict__ p, const float* __restrict__ t, int batch,
                                                         float* __restrict__ raw, float* __restrict__ dY) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const size_t i0 = (size_t)b * R4_OUT + lane * 8;
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const float d = p[i0 + j] - t[i0 + j];
        s += d * d;
        dY[i0 + j] = 2.f * d / (float)batch;
    }
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
    if (lane == 0) raw[b] = s;
}

// BatchNorm backward, the sums: dz = dA where the stored activation is above zero (everywhere without `act`), and the workgroup's
// per-channel sums of dz and dz * xhat in double, part [workgroup][2][32]
__global__ __launch_bounds__(256) void r4l_bn_bwd_sums_kernel(const float* __restrict__ dA, const float* __restrict__ act,
                                                             const float* __restrict__ c, const float* __restrict__ stats,
                                                             float* __restrict__ dz, double* __restrict__ part) {
    __shared__ double red[2][8][CH];
    const int tid = threadIdx.x, ch = tid & 31, g = tid >> 5;
    const float mean = stats[ch], inv = stats[CH + ch];
    const size_t i0 = ((size_t)blockIdx.x * GB * NN + g * 8) * CH + ch;
    double s1 = 0.0, s2 = 0.0;
#pragma unroll
    for (int r = 0; r < 8; r++) {
        const size_t i = i0 + (size_t)r * CH;
        const float d = (!act || act[i] > 0.f) ? dA[i] : 0.f;
        dz[i] = d;
        const float xh = (c[i] - mean) * inv;
        s1 += (double)d;
        s2 += (double)d * (double)xh;
    }
    red[0][g][ch] = s1;
    red[1][g][ch] = s2;
    __syncthreads();
    if (tid < 2 * CH) {
        double s = 0.0;
        for (int k = 0; k < 8; k++) s += red[tid >> 5][k][ch];
        part[(size_t)blockIdx.x * 2 * CH + tid] = s;
    }
}

// BatchNorm backward, the rest, and the conv's data gradient.  dc = gamma * invstd * (dz - mean(dz) - xhat * mean(dz * xhat)); workgroup 0
// writes the BatchNorm weight's gradient sum(dz * xhat) and the bias's sum(dz).  din[s][ci] = sum_tap sum_co dc[s - d(tap)][co] *
// W[tap][ci][co] (+ skip): one wave per board, the k index of an MFMA step is co = 8 (lane >> 4) + j so that a lane's eight weights
// are consecutive.
__global__ __launch_bounds__(256) void r4l_dconv_kernel(const float* __restrict__ dz, const float* __restrict__ c, const float* __restrict__ stats,
                                                       const float* __restrict__ gamma, const double* __restrict__ part, int nparts, int rows,
                                                       const float* __restrict__ W, const float* __restrict__ skip, float* __restrict__ dc,
                                                       float* __restrict__ din, float* __restrict__ g_gamma) {
    __shared__ double tot[2 * CH];
    __shared__ float img[GB][NN + 1][PITCH];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 15, q = lane >> 4;
    sum_partials(part, nparts, tot, tid);
    if (blockIdx.x == 0 && tid < 2 * CH) g_gamma[tid < CH ? CH + tid : tid - CH] = (float)tot[tid];   // [weight, bias] <- [sum dz xhat, sum dz]
    const size_t board = (size_t)blockIdx.x * GB + wave;
    {
        const int ch = lane & 31;
        const float mean = stats[ch], inv = stats[CH + ch], k = gamma[ch] * inv;
        const float m1 = (float)(tot[ch] / rows), m2 = (float)(tot[CH + ch] / rows);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int e = lane + 64 * j;
            const size_t i = board * NN * CH + e;
            const float xh = (c[i] - mean) * inv;
            const float v = k * (dz[i] - m1 - xh * m2);
            img[wave][e >> 5][ch] = v;
            dc[i] = v;
        }
        if (lane < CH) img[wave][NN][lane] = 0.f;
    }
    __syncthreads();
    f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
    for (int tap = 0; tap < 9; tap++) {
        const float* arow = img[wave][tap_row(col, 8 - tap)] + q * 8;
        const float* wr = W + ((size_t)tap * CH + col) * CH + q * 8;
        float w0[8], w1[8];
        *reinterpret_cast<float4*>(w0) = *reinterpret_cast<const float4*>(wr);
        *reinterpret_cast<float4*>(w0 + 4) = *reinterpret_cast<const float4*>(wr + 4);
        *reinterpret_cast<float4*>(w1) = *reinterpret_cast<const float4*>(wr + 16 * CH);
        *reinterpret_cast<float4*>(w1 + 4) = *reinterpret_cast<const float4*>(wr + 16 * CH + 4);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const float av = arow[j];
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w0[j], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av, w1[j], acc[1], 0, 0, 0);
        }
    }
#pragma unroll
    for (int ct = 0; ct < 2; ct++)
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const size_t o = (board * NN + q * 4 + i) * CH + ct * 16 + col;
            din[o] = skip ? acc[ct][i] + skip[o] : acc[ct][i];
        }
}

// weight gradient of one tap over WB boards: part[chunk][tap][ci][co] = sum_rows in[row shifted by the tap][ci] * dc[row][co], one wave,
// four 16x16 tiles, k = the rows in order
__global__ __launch_bounds__(64) void r4l_dw_kernel(const float* __restrict__ in, const float* __restrict__ dc, float* __restrict__ part) {
    const int tap = blockIdx.x, chunk = blockIdx.y, lane = threadIdx.x, col = lane & 15, q = lane >> 4;
    f32x4 acc[2][2];
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int n = 0; n < 2; n++) acc[m][n] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int ks = 0; ks < WB * NN / 4; ks++) {
        const size_t row = (size_t)chunk * WB * NN + ks * 4 + q;
        const int src = tap_row((int)(row & 15), tap);
        float a0 = 0.f, a1 = 0.f;
        if (src < NN) {
            const float* ar = in + ((row & ~(size_t)15) + src) * CH;
            a0 = ar[col];
            a1 = ar[16 + col];
        }
        const float b0 = dc[row * CH + col], b1 = dc[row * CH + 16 + col];
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
    float* o = part + ((size_t)chunk * 9 + tap) * CH * CH;
#pragma unroll
    for (int m = 0; m < 2; m++)
#pragma unroll
        for (int n = 0; n < 2; n++)
#pragma unroll
            for (int i = 0; i < 4; i++) o[(m * 16 + q * 4 + i) * CH + n * 16 + col] = acc[m][n][i];
}

// LayerNorm's affine gradients over GB boards: part[workgroup][0][e] = sum_b dx * xhat, [1][e] = sum_b dx (dx: the first conv's data gradient)
__global__ __launch_bounds__(256) void r4l_ln_bwd_kernel(const float* __restrict__ din, const float* __restrict__ xhat, double* __restrict__ part) {
    for (int e = threadIdx.x; e < R4_IN; e += 256) {
        double s1 = 0.0, s2 = 0.0;
        for (int k = 0; k < GB; k++) {
            const size_t b = (size_t)blockIdx.x * GB + k;
            const float dx = din[(b * NN + (e & 15)) * CH + (e >> 4)];
            s1 += (double)dx * (double)xhat[b * R4_IN + e];
            s2 += (double)dx;
        }
        part[((size_t)blockIdx.x * 2) * R4_IN + e] = s1;
        part[((size_t)blockIdx.x * 2 + 1) * R4_IN + e] = s2;
    }
}

// the partials in order: workgroups 0 .. 36 L - 1 the conv weights' gradients, the next four LayerNorm's, the last the loss
constexpr int FIN_W = L * WSZ / 256, FIN_LN = (2 * R4_IN + 255) / 256;
__global__ __launch_bounds__(256) void r4l_finish_kernel(const float* __restrict__ wpart, int wparts, const double* __restrict__ lnpart, int lnparts,
                                                        const float* __restrict__ raw, int batch, float* __restrict__ G, float* __restrict__ loss) {
    const int blk = blockIdx.x, tid = threadIdx.x;
    if (blk < FIN_W) {
        const int l = blk / (WSZ / 256), i = (blk % (WSZ / 256)) * 256 + tid;
        double s = 0.0;
        for (int p = 0; p < wparts; p++) s += (double)wpart[((size_t)l * wparts + p) * WSZ + i];
        G[R4L_W + (size_t)l * WSZ + i] = (float)s;
    } else if (blk < FIN_W + FIN_LN) {
        const int j = (blk - FIN_W) * 256 + tid;
        if (j >= 2 * R4_IN) return;
        const int which = j / R4_IN, e = j % R4_IN;
        double s = 0.0;
        for (int p = 0; p < lnparts; p++) s += lnpart[((size_t)p * 2 + which) * R4_IN + e];
        G[(which ? R4L_LNB : R4L_LNW) + e] = (float)s;
    } else if (tid == 0) {
        double s = 0.0;
        for (int b = 0; b < batch; b++) s += (double)raw[b];
        loss[0] = (float)(s / batch);
    }
}

int launch_check(const char* what) {
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return tz_fail(TZ_EDEVICE, std::string(what) + ": " + hipGetErrorString(e));
    return TZ_OK;
}

template <typename T>
int dalloc(Rnd4Learn* r, T** p, size_t count) {
    void* q = nullptr;
    if (hipMalloc(&q, count * sizeof(T)) != hipSuccess) return tz_fail(TZ_ENOMEM, "trainer: device allocation failed");
    r->allocs.push_back(q);
    if (hipMemset(q, 0, count * sizeof(T)) != hipSuccess) return tz_fail(TZ_EDEVICE, "trainer: memset failed");
    *p = (T*)q;
    return TZ_OK;
}

const char* const TOWERS[2] = {"rnd_predictor", "rnd_target"};
// (conv, batch norm) paths of layer l below a tower's prefix
std::string conv_path(int l) {
    if (l == 0) return ".input_conv2d";
    if (l == L - 1) return ".last_small_block.conv2d";
    return ".res_block_" + std::to_string((l - 1) / 2) + ((l - 1) & 1 ? ".b" : ".a") + ".conv2d";
}
std::string norm_path(int l) {
    if (l == 0) return ".batch_norm";
    if (l == L - 1) return ".last_small_block.batch_norm";
    return ".res_block_" + std::to_string((l - 1) / 2) + ((l - 1) & 1 ? ".b" : ".a") + ".batch_norm";
}
bool residual(int l) { return !(l & 1) && l >= 2 && l < L - 1; }

// place of a variable below a tower's prefix (tz_rnd4l_find)
bool find_below(const std::string& rest, size_t& off, size_t& count, int& kind, int& ci) {
    kind = 0;
    ci = 0;
    if (rest == ".layer_norm.weight" || rest == ".layer_norm.bias") {
        off = rest == ".layer_norm.weight" ? R4L_LNW : R4L_LNB;
        count = R4_IN;
        return true;
    }
    for (int l = 0; l < L; l++) {
        if (rest == conv_path(l) + ".weight") {
            kind = 1;
            ci = l == 0 ? R4_CIN : CH;
            off = R4L_W + (size_t)l * WSZ;
            count = (size_t)CH * ci * 9;
            return true;
        }
        const std::string n = norm_path(l);
        count = CH;
        if (rest == n + ".weight") return off = R4L_BN + 2 * CH * l, true;
        if (rest == n + ".bias") return off = R4L_BN + 2 * CH * l + CH, true;
        kind = 2;
        if (rest == n + ".running_mean") return off = 2 * CH * l, true;
        if (rest == n + ".running_var") return off = 2 * CH * l + CH, true;
        kind = 0;
    }
    return false;
}

const char* const SUFFIXES[5] = {".weight", ".bias", ".running_mean", ".running_var", nullptr};
// every variable of a tower: f(name below the prefix)
template <typename F>
int for_each_variable(F f) {
    int rc;
    if ((rc = f(std::string(".layer_norm.weight"))) || (rc = f(std::string(".layer_norm.bias")))) return rc;
    for (int l = 0; l < L; l++) {
        if ((rc = f(conv_path(l) + ".weight"))) return rc;
        for (int s = 0; SUFFIXES[s]; s++)
            if ((rc = f(norm_path(l) + SUFFIXES[s]))) return rc;
    }
    return TZ_OK;
}

// reference layout <-> arena layout of one variable
void pack(int kind, int ci_n, const float* data, size_t count, float* dst) {
    if (kind != 1) {
        memcpy(dst, data, count * sizeof(float));
        return;
    }
    for (int tap = 0; tap < 9; tap++)
        for (int ci = 0; ci < CH; ci++)
            for (int co = 0; co < CH; co++) dst[(tap * CH + ci) * CH + co] = ci < ci_n ? data[((size_t)co * ci_n + ci) * 9 + tap] : 0.f;
}
void unpack(int kind, int ci_n, const float* src, size_t count, float* out) {
    if (kind != 1) {
        memcpy(out, src, count * sizeof(float));
        return;
    }
    for (int co = 0; co < CH; co++)
        for (int ci = 0; ci < ci_n; ci++)
            for (int tap = 0; tap < 9; tap++) out[((size_t)co * ci_n + ci) * 9 + tap] = src[(tap * CH + ci) * CH + co];
}
size_t extent(int kind, size_t count) { return kind == 1 ? (size_t)WSZ : count; }

int sync_all(Rnd4Learn* r) {
    TZ_HIP(hipSetDevice(r->device));
    TZ_HIP(hipStreamSynchronize(r->stream));
    return TZ_OK;
}

}  // namespace

int tz_rnd4l_create(int batch, int device, Rnd4Learn** out) {
    if (batch <= 0 || batch % 64) return tz_fail(TZ_EINVAL, "net4_rnd predictor training: batch must be a positive multiple of 64");
    Rnd4Learn* r = new Rnd4Learn();
    r->batch = batch;
    r->device = device;
    const size_t B = (size_t)batch, act = B * NN * CH;
    int rc = TZ_OK;
    do {
        if ((rc = dalloc(r, &r->P, (size_t)R4L_TOTAL)) || (rc = dalloc(r, &r->G, (size_t)R4L_TOTAL)) || (rc = dalloc(r, &r->M1, (size_t)R4L_TOTAL)) ||
            (rc = dalloc(r, &r->M2, (size_t)R4L_TOTAL)) || (rc = dalloc(r, &r->TP, (size_t)R4L_TOTAL)) || (rc = dalloc(r, &r->rs, (size_t)L * 2 * CH)) ||
            (rc = dalloc(r, &r->trs, (size_t)L * 2 * CH)) || (rc = dalloc(r, &r->group, (size_t)R4L_TOTAL / 1024)) ||
            (rc = dalloc(r, &r->xhat, B * R4_IN)) || (rc = dalloc(r, &r->ln[0], act)) || (rc = dalloc(r, &r->ln[1], act)) ||
            (rc = dalloc(r, &r->stats, (size_t)L * 2 * CH)) || (rc = dalloc(r, &r->dY, act)) || (rc = dalloc(r, &r->raw, B)) ||
            (rc = dalloc(r, &r->loss, (size_t)4)) || (rc = dalloc(r, &r->fpart, B / GB * 2 * CH)) || (rc = dalloc(r, &r->bpart, B / GB * 2 * CH)) ||
            (rc = dalloc(r, &r->lnpart, B / GB * 2 * R4_IN)) || (rc = dalloc(r, &r->wpart, (size_t)L * (B / WB) * WSZ)) ||
            (rc = dalloc(r, &r->states, B)) || (rc = dalloc(r, &r->cal_wf, (size_t)2 * L * WSZ)) || (rc = dalloc(r, &r->cal_bias, (size_t)2 * L * CH)) ||
            (rc = dalloc(r, &r->cal_ln, (size_t)4 * R4_IN)) || (rc = dalloc(r, &r->cal_ube, B)) || (rc = dalloc(r, &r->cal_raw, B)) ||
            (rc = dalloc(r, &r->cal_var, B)))
            break;
        for (int l = 0; l < L && !rc; l++)
            (rc = dalloc(r, &r->c[l], act)) || (rc = dalloc(r, &r->a[0][l], act)) || (rc = dalloc(r, &r->a[1][l], act)) ||
                (rc = dalloc(r, &r->dz[l], act)) || (rc = dalloc(r, &r->dc[l], act)) || (rc = dalloc(r, &r->din[l], act));
        if (rc) break;
        if (hipMemset(r->group, 3, R4L_TOTAL / 1024) != hipSuccess || hipStreamCreate(&r->stream) != hipSuccess ||
            hipEventCreateWithFlags(&r->ev_x0, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&r->ev_done, hipEventDisableTiming) != hipSuccess)
            rc = tz_fail(TZ_EDEVICE, "net4_rnd predictor training: stream or event");
    } while (0);
    if (rc) {
        tz_rnd4l_destroy(r);
        return rc;
    }
    *out = r;
    return TZ_OK;
}

void tz_rnd4l_destroy(Rnd4Learn* r) {
    if (!r) return;
    if (r->stream) {
        (void)hipStreamSynchronize(r->stream);
        (void)hipStreamDestroy(r->stream);
    }
    if (r->ev_x0) (void)hipEventDestroy(r->ev_x0);
    if (r->ev_done) (void)hipEventDestroy(r->ev_done);
    for (void* q : r->allocs) (void)hipFree(q);
    delete r;
}

bool tz_rnd4l_find(const std::string& name, size_t& off, size_t& count, int& kind, int& ci) {
    const size_t n = strlen(TOWERS[0]);
    if (name.compare(0, n, TOWERS[0]) != 0) return false;
    return find_below(name.substr(n), off, count, kind, ci);
}

bool tz_rnd4l_present(const TensorStore& st) {
    for (const char* scalar : {"min", "max"}) {
        auto it = st.find(scalar);
        if (it == st.end() || it->second.data.size() != 1) return false;
    }
    for (const char* tower : TOWERS) {
        const int rc = for_each_variable([&](const std::string& rest) {
            size_t off, count;
            int kind, ci;
            find_below(rest, off, count, kind, ci);
            auto it = st.find(tower + rest);
            return it != st.end() && it->second.data.size() == count ? 0 : 1;
        });
        if (rc) return false;
    }
    return true;
}

int tz_rnd4l_upload(Rnd4Learn* r, const TensorStore& st) {
    int rc;
    if ((rc = sync_all(r))) return rc;
    for (int t = 0; t < 2; t++) {
        std::vector<float> arena(R4L_TOTAL, 0.f), running((size_t)L * 2 * CH, 0.f);
        for_each_variable([&](const std::string& rest) {
            size_t off, count;
            int kind, ci;
            find_below(rest, off, count, kind, ci);
            pack(kind, ci, st.at(TOWERS[t] + rest).data.data(), count, (kind == 2 ? running.data() : arena.data()) + off);
            return 0;
        });
        TZ_HIP(hipMemcpy(t ? r->TP : r->P, arena.data(), arena.size() * sizeof(float), hipMemcpyHostToDevice));
        TZ_HIP(hipMemcpy(t ? r->trs : r->rs, running.data(), running.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    return TZ_OK;
}

int tz_rnd4l_download(Rnd4Learn* r, TensorStore& st) {
    int rc;
    if ((rc = sync_all(r))) return rc;
    std::vector<float> arena(R4L_TOTAL), running((size_t)L * 2 * CH);
    TZ_HIP(hipMemcpy(arena.data(), r->P, arena.size() * sizeof(float), hipMemcpyDeviceToHost));
    TZ_HIP(hipMemcpy(running.data(), r->rs, running.size() * sizeof(float), hipMemcpyDeviceToHost));
    for_each_variable([&](const std::string& rest) {
        size_t off, count;
        int kind, ci;
        find_below(rest, off, count, kind, ci);
        HostTensor& h = st[TOWERS[0] + rest];   // present since the feature was enabled: the shape stays
        h.data.resize(count);
        unpack(kind, ci, (kind == 2 ? running.data() : arena.data()) + off, count, h.data.data());
        return 0;
    });
    return TZ_OK;
}

int tz_rnd4l_set(Rnd4Learn* r, const std::string& name, int what, const float* data, size_t count) {
    size_t off, n;
    int kind, ci, rc;
    if (!tz_rnd4l_find(name, off, n, kind, ci)) return tz_fail(TZ_EINVAL, "tz_trainer_set_tensor: unknown tensor " + name);
    float* arena = kind == 2 ? (what == 0 ? r->rs : nullptr) : what == 0 ? r->P : what == 1 ? r->G : what == 2 ? r->M1 : what == 3 ? r->M2 : nullptr;
    if (!arena) return tz_fail(TZ_EINVAL, "tz_trainer_set_tensor: unknown tensor " + name);
    if (count != n) return tz_fail(TZ_EPARSE, "tz_trainer_set_tensor: wrong size for " + name);
    if ((rc = sync_all(r))) return rc;
    std::vector<float> host(extent(kind, n));
    pack(kind, ci, data, n, host.data());
    TZ_HIP(hipMemcpy(arena + off, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice));
    return TZ_OK;
}

int tz_rnd4l_get(Rnd4Learn* r, const std::string& name, int what, float* out, size_t count) {
    size_t off, n;
    int kind, ci, rc;
    if (!tz_rnd4l_find(name, off, n, kind, ci)) return tz_fail(TZ_EINVAL, "tz_trainer_get_tensor: unknown tensor " + name);
    const float* arena = kind == 2 ? (what == 0 ? r->rs : nullptr) : what == 0 ? r->P : what == 1 ? r->G : what == 2 ? r->M1 : what == 3 ? r->M2 : nullptr;
    if (!arena) return tz_fail(TZ_EINVAL, "tz_trainer_get_tensor: unknown tensor " + name);
    if (count != n) return tz_fail(TZ_EPARSE, "tz_trainer_get_tensor: wrong size for " + name);
    if ((rc = sync_all(r))) return rc;
    std::vector<float> host(extent(kind, n));
    TZ_HIP(hipMemcpy(host.data(), arena + off, host.size() * sizeof(float), hipMemcpyDeviceToHost));
    unpack(kind, ci, host.data(), n, out);
    return TZ_OK;
}

int tz_rnd4l_chain(Rnd4Learn* r, const float* x0, int apply) {
    const int B = r->batch, groups = B / GB, rows = B * NN;
    hipStream_t st = r->stream;
    int rc;
    TZ_HIP(hipStreamWaitEvent(st, r->ev_x0, 0));
    r4l_ln_fwd_kernel<<<B, 64, 0, st>>>(x0, r->P, r->TP, r->xhat, r->ln[0], r->ln[1]);
    if ((rc = launch_check("rnd4 layer norm"))) return rc;
    for (int l = 0; l < L; l++) {   // the predictor, training mode
        const float* in = l == 0 ? r->ln[0] : r->a[0][l - 1];
        r4l_conv_fwd_kernel<false><<<groups, 256, 0, st>>>(in, r->P + R4L_W + (size_t)l * WSZ, r->c[l], r->fpart, nullptr, nullptr, nullptr, 0);
        r4l_bn_act_kernel<<<groups, 256, 0, st>>>(r->c[l], r->fpart, groups, rows, r->P + R4L_BN + 2 * CH * l, residual(l) ? r->a[0][l - 2] : nullptr,
                                                  l < L - 1, r->a[0][l], r->stats + 2 * CH * l, r->rs + 2 * CH * l, apply ? 1 : 0);
    }
    if ((rc = launch_check("rnd4 predictor forward"))) return rc;
    for (int l = 0; l < L; l++) {   // the target, eval mode
        const float* in = l == 0 ? r->ln[1] : r->a[1][l - 1];
        r4l_conv_fwd_kernel<true><<<groups, 256, 0, st>>>(in, r->TP + R4L_W + (size_t)l * WSZ, r->a[1][l], nullptr, r->TP + R4L_BN + 2 * CH * l,
                                                         r->trs + 2 * CH * l, residual(l) ? r->a[1][l - 2] : nullptr, l < L - 1);
    }
    r4l_distance_kernel<<<B, 64, 0, st>>>(r->a[0][L - 1], r->a[1][L - 1], B, r->raw, r->dY);
    if ((rc = launch_check("rnd4 target forward"))) return rc;
    for (int l = L - 1; l >= 0; l--) {
        const float* in = l == 0 ? r->ln[0] : r->a[0][l - 1];
        const float* W = r->P + R4L_W + (size_t)l * WSZ;
        r4l_bn_bwd_sums_kernel<<<groups, 256, 0, st>>>(l == L - 1 ? r->dY : r->din[l + 1], l < L - 1 ? r->a[0][l] : nullptr, r->c[l],
                                                       r->stats + 2 * CH * l, r->dz[l], r->bpart);
        // the block's input also feeds the residual add two layers on: its gradient there is that layer's dz
        const float* skip = (l & 1) && l + 1 < L - 1 ? r->dz[l + 1] : nullptr;
        r4l_dconv_kernel<<<groups, 256, 0, st>>>(r->dz[l], r->c[l], r->stats + 2 * CH * l, r->P + R4L_BN + 2 * CH * l, r->bpart, groups, rows, W, skip,
                                                 r->dc[l], r->din[l], r->G + R4L_BN + 2 * CH * l);
        r4l_dw_kernel<<<dim3(9, B / WB), 64, 0, st>>>(in, r->dc[l], r->wpart + (size_t)l * (B / WB) * WSZ);
    }
    r4l_ln_bwd_kernel<<<groups, 256, 0, st>>>(r->din[0], r->xhat, r->lnpart);
    r4l_finish_kernel<<<FIN_W + FIN_LN + 1, 256, 0, st>>>(r->wpart, B / WB, r->lnpart, groups, r->raw, B, r->G, r->loss);
    return launch_check("rnd4 backward");
}

int tz_rnd4l_activation(Rnd4Learn* r, int which, int layer, float* out, size_t cap) {
    if (which < 0 || which > 1 || layer < 0 || layer > (which == 0 ? 2 * L : L))
        return tz_fail(TZ_EINVAL, "tz_trainer_rnd4_activation: no such tower or layer");
    const size_t B = (size_t)r->batch, real = layer == 0 ? B * R4_IN : B * NN * CH;
    if (cap < real) return tz_fail(TZ_EINVAL, "tz_trainer_rnd4_activation: the buffer is too small");
    int rc;
    if ((rc = sync_all(r))) return rc;
    if (layer > 0) {
        TZ_HIP(hipMemcpy(out, layer > L ? r->c[layer - L - 1] : r->a[which][layer - 1], real * sizeof(float), hipMemcpyDeviceToHost));
        return TZ_OK;
    }
    std::vector<float> host(B * NN * CH);
    TZ_HIP(hipMemcpy(host.data(), r->ln[which], host.size() * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t b = 0; b < B; b++)
        for (int e = 0; e < R4_IN; e++) out[b * R4_IN + e] = host[(b * NN + (e & 15)) * CH + (e >> 4)];
    return TZ_OK;
}

// update_rnd's two extremes through the inference library's f32 tower: the current variables folded as build_weights folds a model's
// (scale = weight / sqrt(running_var + eps) into the conv weights, bias - running_mean * scale a bias), so that the answer is what the
// saved model returns in TZ_PREC_F32.  found[0] = min over early, found[1] = max over late.
int tz_rnd4l_calibrate(Rnd4Learn* r, const tz_state* early, int n_early, const tz_state* late, int n_late, float* found) {
    int rc;
    if ((rc = sync_all(r))) return rc;
    std::vector<float> wf((size_t)2 * L * WSZ), fb((size_t)2 * L * CH), ln((size_t)4 * R4_IN);
    for (int t = 0; t < 2; t++) {
        std::vector<float> arena(R4L_TOTAL), running((size_t)L * 2 * CH);
        TZ_HIP(hipMemcpy(arena.data(), t ? r->TP : r->P, arena.size() * sizeof(float), hipMemcpyDeviceToHost));
        TZ_HIP(hipMemcpy(running.data(), t ? r->trs : r->rs, running.size() * sizeof(float), hipMemcpyDeviceToHost));
        memcpy(&ln[(size_t)t * 2 * R4_IN], &arena[R4L_LNW], R4_IN * sizeof(float));
        memcpy(&ln[(size_t)(t * 2 + 1) * R4_IN], &arena[R4L_LNB], R4_IN * sizeof(float));
        for (int l = 0; l < L; l++) {
            const size_t li = (size_t)t * L + l;
            const float *g = &arena[R4L_BN + 2 * CH * l], *b = g + CH, *mean = &running[2 * CH * l], *var = mean + CH;
            float scale[CH];
            for (int co = 0; co < CH; co++) {
                const float s = g[co] / sqrtf(var[co] + 1e-5f);
                scale[co] = s;
                fb[li * CH + co] = b[co] - mean[co] * s;
            }
            const float* w = &arena[R4L_W + (size_t)l * WSZ];
            for (int i = 0; i < WSZ; i++) wf[li * WSZ + i] = w[i] * scale[i % CH];
        }
    }
    TZ_HIP(hipMemcpy(r->cal_wf, wf.data(), wf.size() * sizeof(float), hipMemcpyHostToDevice));
    TZ_HIP(hipMemcpy(r->cal_bias, fb.data(), fb.size() * sizeof(float), hipMemcpyHostToDevice));
    TZ_HIP(hipMemcpy(r->cal_ln, ln.data(), ln.size() * sizeof(float), hipMemcpyHostToDevice));
    const int B = r->batch;
    std::vector<float> raw(B);
    found[0] = INFINITY;
    found[1] = -INFINITY;
    for (int set = 0; set < 2; set++) {
        const tz_state* states = set ? late : early;
        const int count = set ? n_late : n_early;
        for (int c0 = 0; c0 < count; c0 += B) {
            const int cnt = std::min(B, count - c0);
            TZ_HIP(hipMemcpyAsync(r->states, states + c0, sizeof(tz_state) * cnt, hipMemcpyHostToDevice, r->stream));
            if ((rc = tz_nn_launch_rnd4(true, r->states, nullptr, nullptr, cnt, cnt, nullptr, r->cal_wf, r->cal_bias, r->cal_ln, r->cal_ube, 0.f, 1.f,
                                        r->cal_raw, r->cal_var, r->stream)))
                return rc;
            if ((rc = launch_check("rnd4 calibrate"))) return rc;
            TZ_HIP(hipMemcpyAsync(raw.data(), r->cal_raw, sizeof(float) * cnt, hipMemcpyDeviceToHost, r->stream));
            TZ_HIP(hipStreamSynchronize(r->stream));
            for (int i = 0; i < cnt; i++) {
                if (set == 0) found[0] = fminf(found[0], raw[i]);
                else found[1] = fmaxf(found[1], raw[i]);
            }
        }
    }
    return TZ_OK;
}
