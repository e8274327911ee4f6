// tz_nn_rnd4.hip — the two RND towers of TZ_ARCH_NET4_RND (net4_rnd.rs:126-166, 210-230, 289-297) and the variance rule, one launch.
// A unit of its own on tz_nn.hip's device encoder (plane_value): nothing another architecture runs is compiled here.
//
// Each tower: LayerNorm([28,4,4]) with an elementwise affine, conv 3x3 28->32 + BN + ReLU, four ResidualBlock(32, 32)
// (relu(conv+BN(relu(conv+BN(x))) + x), residual.rs:50-62), SmallBlock(32, 32) without ReLU, 512 outputs.  BatchNorm is folded on the
// host (scale into the weights, the rest into a bias).  raw = sum_512 (predictor - target)^2, local = clamp((raw - min) / (max - min),
// 0, 1) * 4, variance = clamp(max(e^ube, local), 0, 4) with tz_expf.  The unit compiles without FMA contraction and with correctly
// rounded division, so a caller restates `variance` from raw, ube, min and max bit for bit.
//
// rnd4_tower_mfma_kernel (every precision but TZ_PREC_F32): one wave per workgroup, R4_BOARDS boards per wave.  A board's 16 squares
// are the 16 rows of a v_mfma_f32_16x16x32_f16 tile, a k-step is one tap's 32 input channels, the 32 output channels are two column
// tiles: 18 MFMAs per board and layer.  A layer's 18 KB of fp16 weights arrive from L2 in fragment order ([tap][column tile][lane][8])
// and stay in registers for the wave's boards.  Activations live in LDS as fp16, [square][32 channels] per board in two buffers (the
// block's input X and its middle T) with a zero row for the taps that leave the board; accumulation, bias, the residual add and ReLU
// are fp32.  The last layer's outputs are not rounded: the difference, its square and the 512-term sum are fp32 (each lane its 8
// elements in order, then an xor butterfly over the wave).  A board's arithmetic never meets another board's, so its raw has the
// same bits at any slot, batch size and precision.
//
// rnd4_tower_f32_kernel (TZ_PREC_F32): the same graph in plain fp32, one workgroup of 512 threads (square, channel) per board.
#define TZ_NN_SPLIT_TU 1
#define TZ_NN_RND4_TU 1
#include "tz_nn.hip"
#include "tz_nn_rnd4.h"

namespace {

constexpr int R4_ROWB = 64;                   // one square's 32 fp16 channels
constexpr int R4_BUF = (R4_NN + 1) * R4_ROWB;   // 16 squares and the zero row
constexpr float R4_EPS = 1e-5f;               // tch LayerNormConfig::default

struct Rnd4Args {
    const tz_state* states;
    const int32_t* gidx;
    const int32_t* count_dev;
    int count_host;
    const uint16_t* w;    // fp16 [tower][layer][tap][column tile][lane][8]
    const float* wf;      // fp32 [tower][layer][tap][ci][co]
    const float* bias;    // [tower][layer][32]
    const float* ln;      // [tower][weight, bias][plane * 16 + square]
    const float* ube;
    float rmin, rmax;
    float* raw;
    float* variance;
};

// net4_rnd.rs:225-230, 289-297
__device__ __forceinline__ float rnd4_variance(float raw, float ube, float rmin, float rmax) {
    float local = (raw - rmin) / (rmax - rmin);
    local = fminf(fmaxf(local, 0.f), 1.f) * 4.0f;
    return fminf(fmaxf(fmaxf(tz_expf(ube), local), 0.f), 4.f);
}

__device__ __forceinline__ int rnd4_tap_row(int square, int tap) {   // the source square of a tap, 16 (the zero row) off the board
    const int y = (square >> 2) + tap / 3 - 1, x = (square & 3) + tap % 3 - 1;
    return (y >= 0 && y < 4 && x >= 0 && x < 4) ? y * 4 + x : R4_NN;
}

__global__ __launch_bounds__(64) void rnd4_tower_mfma_kernel(Rnd4Args a) {
    __shared__ __attribute__((aligned(16))) unsigned char img[R4_BOARDS][2][R4_BUF];   // [board][X, T]
    __shared__ tz_state sh[R4_BOARDS];
    const int count = a.count_dev ? *a.count_dev : a.count_host;
    const int lane = threadIdx.x, pos0 = blockIdx.x * R4_BOARDS;
    if (pos0 >= count) return;
    // a tail workgroup computes its last valid board again in the empty slots and writes nothing for them
#pragma unroll
    for (int b = 0; b < R4_BOARDS; b++) {
        const int p = min(pos0 + b, count - 1);
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.states + (a.gidx ? a.gidx[p] : p));
        uint32_t* dst = reinterpret_cast<uint32_t*>(&sh[b]);
        for (int i = lane; i < (int)(sizeof(tz_state) / 4); i += 64) dst[i] = src[i];
    }
    for (int i = lane; i < R4_BOARDS * 2 * (R4_ROWB / 4); i += 64)
        reinterpret_cast<uint32_t*>(&img[0][0][0] + (i / (R4_ROWB / 4)) * R4_BUF + R4_NN * R4_ROWB)[i % (R4_ROWB / 4)] = 0u;
    __syncthreads();

    // LayerNorm statistics in fp32 (population variance over the 448 elements, two passes): lane holds elements lane + 64 k, each
    // lane sums its seven in order, then the butterfly
    float xh[R4_BOARDS][7];
#pragma unroll
    for (int b = 0; b < R4_BOARDS; b++) {
        const tz_state* s = &sh[b];
        const int fd = state_flat_diff<4>(s);
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            const int e = lane + 64 * k;
            xh[b][k] = plane_value<4>(s, e & 15, e >> 4, fd);
            sum += xh[b][k];
        }
        for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
        const float mean = sum / (float)R4_IN;
        float sq = 0.f;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            xh[b][k] -= mean;
            sq += xh[b][k] * xh[b][k];
        }
        for (int d = 32; d >= 1; d >>= 1) sq += __shfl_xor(sq, d);
        const float rstd = 1.0f / sqrtf(sq / (float)R4_IN + R4_EPS);
#pragma unroll
        for (int k = 0; k < 7; k++) xh[b][k] *= rstd;
    }

    int aoff[9];   // this lane's A fragment of every tap: row = square lane & 15 shifted by the tap, channels 8 (lane >> 4) ...
#pragma unroll
    for (int tap = 0; tap < 9; tap++) aoff[tap] = rnd4_tap_row(lane & 15, tap) * R4_ROWB + (lane >> 4) * 16;
    const int col = lane & 15, row0 = (lane >> 4) * 4;   // C/D: column = lane & 15, rows 4 (lane >> 4) + i

    float fin[R4_BOARDS][8];
#pragma unroll 1
    for (int t = 0; t < 2; t++) {   // 0: rnd_predictor, 1: rnd_target
        const float* lw = a.ln + t * 2 * R4_IN;
        const float* lb = lw + R4_IN;
#pragma unroll
        for (int k = 0; k < 8; k++) {   // the affine output into T; channels 28..31 (k = 7) are zero
            const int e = lane + 64 * k;
            const float w = k < 7 ? lw[e] : 0.f, bb = k < 7 ? lb[e] : 0.f;
#pragma unroll
            for (int b = 0; b < R4_BOARDS; b++) {
                const float v = k < 7 ? xh[b][k] * w + bb : 0.f;
                *reinterpret_cast<_Float16*>(&img[b][1][(e & 15) * R4_ROWB + (e >> 4) * 2]) = Elem<_Float16>::cvt(v);
            }
        }
        __syncthreads();
#pragma unroll 1
        for (int l = 0; l < R4_LAYERS; l++) {
            const uint16_t* wl = a.w + (size_t)(t * R4_LAYERS + l) * R4_LAYER_HALVES;
            f16x8 wfrag[9][2];
#pragma unroll
            for (int tap = 0; tap < 9; tap++)
#pragma unroll
                for (int ct = 0; ct < 2; ct++) wfrag[tap][ct] = *reinterpret_cast<const f16x8*>(wl + ((tap * 2 + ct) * 64 + lane) * 8);
            const float* bl = a.bias + (t * R4_LAYERS + l) * R4_CH;
            const float bias[2] = {bl[col], bl[16 + col]};
            // layer 0 reads the LayerNorm output in T; a block's first conv reads X and writes T, its second reads T, adds X, writes X
            const int srcb = (l & 1) ? 0 : 1, dstb = srcb ^ 1;
            const bool residual = !(l & 1) && l >= 2;
#pragma unroll
            for (int b = 0; b < R4_BOARDS; b++) {
                const unsigned char* src = &img[b][0][0] + srcb * R4_BUF;
                unsigned char* dst = &img[b][0][0] + dstb * R4_BUF;
                f32x4 acc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
                for (int tap = 0; tap < 9; tap++) {
                    const f16x8 af = *reinterpret_cast<const f16x8*>(src + aoff[tap]);
                    acc[0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, wfrag[tap][0], acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af, wfrag[tap][1], acc[1], 0, 0, 0);
                }
                if (l < R4_LAYERS - 1) {
#pragma unroll
                    for (int ct = 0; ct < 2; ct++)
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            _Float16* at = reinterpret_cast<_Float16*>(dst + (row0 + i) * R4_ROWB + (ct * 16 + col) * 2);
                            float v = acc[ct][i] + bias[ct];
                            if (residual) v += (float)*at;
                            *at = Elem<_Float16>::relu_cvt(v);
                        }
                } else if (t == 0) {
#pragma unroll
                    for (int ct = 0; ct < 2; ct++)
#pragma unroll
                        for (int i = 0; i < 4; i++) fin[b][ct * 4 + i] = acc[ct][i] + bias[ct];
                } else {
                    float s = 0.f;
#pragma unroll
                    for (int ct = 0; ct < 2; ct++)
#pragma unroll
                        for (int i = 0; i < 4; i++) {
                            const float d = fin[b][ct * 4 + i] - (acc[ct][i] + bias[ct]);
                            s += d * d;
                        }
                    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d);
                    if (lane == 0 && pos0 + b < count) {
                        a.raw[pos0 + b] = s;
                        a.variance[pos0 + b] = rnd4_variance(s, a.ube[pos0 + b], a.rmin, a.rmax);
                    }
                }
            }
            __syncthreads();
        }
    }
}

// a sum over the workgroup's 512 threads in a fixed tree
__device__ __forceinline__ float rnd4_block_sum(float v, float* red, int tid) {
    red[tid] = v;
    __syncthreads();
    for (int stride = 256; stride > 0; stride >>= 1) {
        if (tid < stride) red[tid] += red[tid + stride];
        __syncthreads();
    }
    const float r = red[0];
    __syncthreads();
    return r;
}

__global__ __launch_bounds__(512) void rnd4_tower_f32_kernel(Rnd4Args a) {
    __shared__ float img[2][R4_NN + 1][R4_CH];   // [X, T][square or the zero row][channel]
    __shared__ float red[512];
    __shared__ tz_state sh;
    const int count = a.count_dev ? *a.count_dev : a.count_host;
    const int pos = blockIdx.x, tid = threadIdx.x;
    if (pos >= count) return;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(a.states + (a.gidx ? a.gidx[pos] : pos));
        uint32_t* dst = reinterpret_cast<uint32_t*>(&sh);
        for (int i = tid; i < (int)(sizeof(tz_state) / 4); i += 512) dst[i] = src[i];
    }
    if (tid < 2 * R4_CH) img[tid >> 5][R4_NN][tid & 31] = 0.f;
    __syncthreads();
    // thread = element plane * 16 + square of the LayerNorm (planes 28..31: the conv's zero padding), and (square, channel) of a conv
    const bool real = tid < R4_IN;
    const int es = tid & 15, ec = tid >> 4;
    const float x = real ? plane_value<4>(&sh, es, ec, state_flat_diff<4>(&sh)) : 0.f;
    const float mean = rnd4_block_sum(x, red, tid) / (float)R4_IN;
    const float dm = real ? x - mean : 0.f;
    const float var = rnd4_block_sum(dm * dm, red, tid) / (float)R4_IN;
    const float xhat = dm * (1.0f / sqrtf(var + R4_EPS));
    const int s = tid >> 5, c = tid & 31;
    int rows[9];
#pragma unroll
    for (int tap = 0; tap < 9; tap++) rows[tap] = rnd4_tap_row(s, tap);
    float fin = 0.f;
    for (int t = 0; t < 2; t++) {
        img[1][es][ec] = real ? xhat * a.ln[t * 2 * R4_IN + tid] + a.ln[(t * 2 + 1) * R4_IN + tid] : 0.f;
        __syncthreads();
        for (int l = 0; l < R4_LAYERS; l++) {
            const int srcb = (l & 1) ? 0 : 1, dstb = srcb ^ 1;
            const float* w = a.wf + (size_t)(t * R4_LAYERS + l) * 9 * R4_CH * R4_CH;
            float acc = 0.f;
            for (int tap = 0; tap < 9; tap++)
                for (int ci = 0; ci < R4_CH; ci++) acc = fmaf(img[srcb][rows[tap]][ci], w[(tap * R4_CH + ci) * R4_CH + c], acc);
            float v = acc + a.bias[(t * R4_LAYERS + l) * R4_CH + c];
            if (l < R4_LAYERS - 1) {
                if (!(l & 1) && l >= 2) v += img[dstb][s][c];
                img[dstb][s][c] = v > 0.f ? v : 0.f;
                __syncthreads();
            } else if (t == 0) {
                fin = v;
            } else {
                const float d = fin - v;
                const float raw = rnd4_block_sum(d * d, red, tid);
                if (tid == 0) {
                    a.raw[pos] = raw;
                    a.variance[pos] = rnd4_variance(raw, a.ube[pos], a.rmin, a.rmax);
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace

int tz_nn_launch_rnd4(bool f32, const tz_state* states, const int32_t* gidx, const int32_t* count_dev, int count_host, int max_positions,
                      const uint16_t* w, const float* wf, const float* bias, const float* ln, const float* ube, float rmin, float rmax,
                      float* raw, float* variance, hipStream_t st) {
    if (!states || !bias || !ln || !ube || !raw || !variance || (f32 ? !wf : !w))
        return tz_fail(TZ_EINVAL, "RND towers: the kernel for this network's weights is missing");
    if (max_positions <= 0) return TZ_OK;
    Rnd4Args a{states, gidx, count_dev, count_host, w, wf, bias, ln, ube, rmin, rmax, raw, variance};
    if (f32) rnd4_tower_f32_kernel<<<max_positions, 512, 0, st>>>(a);
    else rnd4_tower_mfma_kernel<<<(max_positions + R4_BOARDS - 1) / R4_BOARDS, 64, 0, st>>>(a);
    return TZ_OK;
}
