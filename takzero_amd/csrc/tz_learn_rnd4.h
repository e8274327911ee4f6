// tz_learn_rnd4.h — training net4_rnd's predictor tower beside the trunk's step (tz_learn_rnd4.hip): the device state and the calls
// tz_learn.hip makes.  Everything is fp32, sums across workgroups are per-workgroup partials added in a fixed order.
#pragma once
#include <string>
#include <vector>

#include "tz_nn.h"
#include "tz_nn_rnd4.h"

// One arena per kind (parameters P, gradients G, Adam moments M1 / M2), whole Adam blocks of 1024:
//   LayerNorm weight [plane * 16 + square] at R4L_LNW, bias at R4L_LNB; BatchNorm weight of layer l at R4L_BN + 64 l, bias 32 further;
//   conv weight of layer l at R4L_W + l * R4L_WSZ as [tap][ci (32, the first layer's 28..31 zero)][co].
constexpr int R4L_LNW = 0, R4L_LNB = R4_IN, R4L_BN = 1024, R4L_W = 2048, R4L_WSZ = 9 * R4_CH * R4_CH;
constexpr int R4L_TOTAL = R4L_W + R4_LAYERS * R4L_WSZ;   // 94208 = 92 * 1024
constexpr int R4L_GROUP = 4;     // boards per workgroup = boards per partial sum of the batch statistics
constexpr int R4L_WBOARDS = 16;  // boards per partial sum of a weight gradient

struct Rnd4Learn {
    bool on = false, have_last = false;
    int batch = 0, device = 0, t_step = 0;   // t_step: Adam steps of the predictor's group (it may be enabled mid-run)
    float last_loss = 0.f;
    float *P = nullptr, *G = nullptr, *M1 = nullptr, *M2 = nullptr;   // the predictor's arenas
    float* TP = nullptr;                                              // the target's parameters, same layout; never written by a kernel
    float *rs = nullptr, *trs = nullptr;                              // running statistics [layer][mean, var][32]: predictor, target
    uint8_t* group = nullptr;                                         // adam_kernel's group per block: all 3
    float* xhat = nullptr;                                            // [batch][448] LayerNorm's normalised input
    float* ln[2] = {nullptr, nullptr};                                // [tower][batch * 16][32] LayerNorm output, channels 28..31 zero
    float* c[R4_LAYERS] = {};                                         // predictor, before BatchNorm [batch * 16][32]
    float* a[2][R4_LAYERS] = {};                                      // [tower] after BatchNorm, residual and ReLU
    float* stats = nullptr;                                           // [layer][mean, invstd][32] of the batch
    float *dz[R4_LAYERS] = {}, *dc[R4_LAYERS] = {}, *din[R4_LAYERS] = {};   // gradients at a layer's BatchNorm output, conv output, input
    float *dY = nullptr, *raw = nullptr, *loss = nullptr;
    double *fpart = nullptr, *bpart = nullptr, *lnpart = nullptr;     // [batch / 4][2][32] twice, [batch / 4][2][448]
    float* wpart = nullptr;                                           // [layer][batch / 16][tap][ci][co]
    // calibration: the inference library's f32 tower on folded weights
    tz_state* states = nullptr;
    float *cal_wf = nullptr, *cal_bias = nullptr, *cal_ln = nullptr, *cal_ube = nullptr, *cal_raw = nullptr, *cal_var = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev_x0 = nullptr, ev_done = nullptr;
    std::vector<void*> allocs;
};

int tz_rnd4l_create(int batch, int device, Rnd4Learn** out);
void tz_rnd4l_destroy(Rnd4Learn* r);
bool tz_rnd4l_present(const TensorStore& st);                    // both towers, min and max with the right sizes
int tz_rnd4l_upload(Rnd4Learn* r, const TensorStore& st);        // both towers' variables to the device (gradients and moments stay)
int tz_rnd4l_download(Rnd4Learn* r, TensorStore& st);            // the predictor's current variables into the store
// `rnd_predictor.*` name -> place.  kind 0: a vector in the arenas, 1: a conv weight [co][ci][3][3] in the arenas, 2: a running
// statistic (off into rs, parameters only).  false for any other name.
bool tz_rnd4l_find(const std::string& name, size_t& off, size_t& count, int& kind, int& ci);
int tz_rnd4l_set(Rnd4Learn* r, const std::string& name, int what, const float* data, size_t count);
int tz_rnd4l_get(Rnd4Learn* r, const std::string& name, int what, float* out, size_t count);
// forward of both towers, loss and every gradient on r->stream, which first waits for ev_x0 (recorded by the caller once x0 is queued);
// apply: the running statistics move.  The caller launches Adam on r->stream and records ev_done.
int tz_rnd4l_chain(Rnd4Learn* r, const float* x0, int apply);
int tz_rnd4l_activation(Rnd4Learn* r, int which, int layer, float* out, size_t cap);
int tz_rnd4l_calibrate(Rnd4Learn* r, const tz_state* early, int n_early, const tz_state* late, int n_late, float* found);
