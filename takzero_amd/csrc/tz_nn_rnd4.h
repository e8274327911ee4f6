// tz_nn_rnd4.h — the RND towers of TZ_ARCH_NET4_RND (tz_nn_rnd4.hip): shapes of the device weights and the launch.
#pragma once
#include "tz_engine.h"

constexpr int R4_NN = 16, R4_CIN = 28, R4_CH = 32;   // a 4x4 board's squares and input planes, RND_FILTERS (net4_rnd.rs:128)
constexpr int R4_LAYERS = 10;                        // input conv, 4 residual blocks of two, last SmallBlock (net4_rnd.rs:126-166)
constexpr int R4_IN = R4_CIN * R4_NN, R4_OUT = R4_CH * R4_NN;   // 448 LayerNorm elements, 512 outputs
constexpr int R4_BOARDS = 4;                         // boards per workgroup of the MFMA form
constexpr int R4_LAYER_HALVES = 9 * 2 * 64 * 8;      // a layer's fp16 weights in fragment order: [tap][column tile][lane][8]

// Both towers, raw[slot] = sum_512 (predictor - target)^2 and variance[slot] (net4_rnd.rs:210-230, 289-297) for the valid slots, one
// launch on `st`.  w: fp16 fragments [tower][layer][R4_LAYER_HALVES] (the MFMA form), wf: fp32 [tower][layer][tap][ci][co] (f32),
// bias: [tower][layer][32], ln: [tower][weight, bias][448]; tower 0 is rnd_predictor.
int tz_nn_launch_rnd4(bool f32, const tz_state* states, const int32_t* gidx, const int32_t* count_dev, int count_host, int max_positions,
                      const uint16_t* w, const float* wf, const float* bias, const float* ln, const float* ube, float rmin, float rmax,
                      float* raw, float* variance, hipStream_t st);
