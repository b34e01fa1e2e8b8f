// extern "C" surface of libdfd_hip.so (declared in include/dfd_hip.h).
#include "../../include/dfd_hip.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "cnnlstm.h"
#include "head.h"
#include "plan.h"
#include "rn16.h"
#include "rnn.h"
#include "test_seams.h"
#include "vit.h"

namespace dfd {
static thread_local std::string g_err;
void set_error(const char* msg, const char* file, int line) {
  char buf[512];
  const char* base = strrchr(file, '/');
  snprintf(buf, sizeof(buf), "%s (%s:%d)", msg, base ? base + 1 : file, line);
  g_err = buf;
}
}  // namespace dfd

// A plan is shared by every call of one model at one shape; its host-side enqueue state
// (pending BN-stat rows, probe events) is guarded so calls from several threads serialise their
// ENQUEUE (the kernels still run asynchronously on each caller's stream).
struct dfd_b0_plan {
  dfd::Plan p;
  std::mutex mu;
};

#define DFD_GUARD_BEGIN try {
#define DFD_GUARD_END                                        \
  }                                                          \
  catch (const std::exception& e) {                          \
    dfd::set_error(e.what(), __FILE__, __LINE__);            \
    return -1;                                               \
  }                                                          \
  catch (...) {                                              \
    dfd::set_error("unknown C++ exception", __FILE__, __LINE__); \
    return -1;                                               \
  }

extern "C" {

const char* dfd_last_error(void) { return dfd::g_err.c_str(); }
int dfd_version(void) { return 100; }

int dfd_b0_tensor_count(void) { return (int)dfd::b0_tensor_table().size(); }

int dfd_b0_tensor_info(int idx, char* name, int cap, int* kind, int* ndim, int64_t* shape4) {
  const auto& t = dfd::b0_tensor_table();
  if (idx < 0 || idx >= (int)t.size()) { dfd::set_error("tensor index out of range", __FILE__, __LINE__); return -1; }
  const auto& s = t[idx];
  if (name && cap > 0) {
    strncpy(name, s.name.c_str(), cap - 1);
    name[cap - 1] = 0;
  }
  if (kind) *kind = s.kind;
  if (ndim) *ndim = (int)s.shape.size();
  if (shape4)
    for (int i = 0; i < 4; ++i) shape4[i] = i < (int)s.shape.size() ? s.shape[i] : 1;
  return 0;
}

int dfd_b0_plan_create(int frames, int height, int width, int dtype, dfd_b0_plan** out) {
  DFD_GUARD_BEGIN
  if (!out) { dfd::set_error("null out", __FILE__, __LINE__); return -1; }
  auto* h = new (std::nothrow) dfd_b0_plan();
  if (!h) { dfd::set_error("out of host memory", __FILE__, __LINE__); return -1; }
  if (dfd::plan_build(h->p, frames, height, width, dtype) != 0) { delete h; return -1; }
  *out = h;
  return 0;
  DFD_GUARD_END
}

void dfd_b0_plan_destroy(dfd_b0_plan* plan) {
  if (!plan) return;
  dfd::plan_free(plan->p);
  delete plan;
}

int64_t dfd_b0_workspace_bytes(const dfd_b0_plan* plan) { return plan ? plan->p.ws_bytes : -1; }

int dfd_b0_bind(dfd_b0_plan* plan, const int64_t* offsets, int n) {
  DFD_GUARD_BEGIN
  if (!plan || !offsets) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  std::lock_guard<std::mutex> lk(plan->mu);
  return dfd::plan_bind(plan->p, offsets, n);
  DFD_GUARD_END
}

static bool input_fmt(int x_format, const float* norm6, dfd::InputFmt* in) {
  *in = dfd::InputFmt{};
  if (x_format == DFD_INPUT_F32) return true;
  if (x_format != DFD_INPUT_U8) { dfd::set_error("bad input format", __FILE__, __LINE__); return false; }
  in->u8 = 1;
  for (int c = 0; c < 3; ++c) {
    in->mean[c] = norm6 ? norm6[c] : 0.f;
    in->stdv[c] = norm6 ? norm6[3 + c] : 1.f;
    if (!(in->stdv[c] != 0.f)) { dfd::set_error("input normalisation: std must be nonzero", __FILE__, __LINE__); return false; }
  }
  return true;
}

int dfd_b0_forward_ex(dfd_b0_plan* plan, void* stream, const void* x, int x_format, const int64_t* xs,
                      const float* norm6, const float* params, float* bn_buffers, void* workspace, float* features,
                      int training, float momentum) {
  DFD_GUARD_BEGIN
  if (!plan || !x || !xs || !params || !bn_buffers || !workspace || !features) {
    dfd::set_error("null argument", __FILE__, __LINE__);
    return -1;
  }
  dfd::InputFmt in;
  if (!input_fmt(x_format, norm6, &in)) return -1;
  std::lock_guard<std::mutex> lk(plan->mu);
  return dfd::plan_forward(plan->p, (hipStream_t)stream, x, xs, in, params, bn_buffers, (char*)workspace, features,
                           training, momentum);
  DFD_GUARD_END
}

int dfd_b0_forward(dfd_b0_plan* plan, void* stream, const float* x, const int64_t* xs, const float* params,
                   float* bn_buffers, void* workspace, float* features, int training, float momentum) {
  return dfd_b0_forward_ex(plan, stream, x, DFD_INPUT_F32, xs, nullptr, params, bn_buffers, workspace, features,
                           training, momentum);
}

int dfd_b0_backward_ex(dfd_b0_plan* plan, void* stream, const void* x, int x_format, const int64_t* xs,
                       const float* norm6, const float* dfeatures, const float* params, void* workspace, float* grads,
                       int training, int seg_begin, int seg_end, int accumulate) {
  DFD_GUARD_BEGIN
  if (!plan || !x || !xs || !dfeatures || !params || !workspace || !grads) {
    dfd::set_error("null argument", __FILE__, __LINE__);
    return -1;
  }
  dfd::InputFmt in;
  if (!input_fmt(x_format, norm6, &in)) return -1;
  std::lock_guard<std::mutex> lk(plan->mu);
  return dfd::plan_backward_x(plan->p, (hipStream_t)stream, x, xs, in, dfeatures, params, (char*)workspace, grads,
                              training, seg_begin, seg_end, accumulate);
  DFD_GUARD_END
}

int dfd_b0_backward(dfd_b0_plan* plan, void* stream, const float* x, const int64_t* xs, const float* dfeatures,
                    const float* params, void* workspace, float* grads, int training, int seg_begin, int seg_end,
                    int accumulate) {
  return dfd_b0_backward_ex(plan, stream, x, DFD_INPUT_F32, xs, nullptr, dfeatures, params, workspace, grads,
                            training, seg_begin, seg_end, accumulate);
}

int dfd_b0_plan_set_tuning(dfd_b0_plan* plan, const char* key, int64_t value) {
  if (!plan || !key) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  for (int k = 0; k < dfd::TK_COUNT; ++k)
    if (strcmp(key, dfd::kTuneNames[k]) == 0) {
      std::lock_guard<std::mutex> lk(plan->mu);
      plan->p.tune.v[k] = value;
      return 0;
    }
  dfd::set_error("plan_set_tuning: unknown key", __FILE__, __LINE__);
  return -1;
}

int dfd_b0_segment_count(void) { return dfd::kNumSegments; }

int dfd_b0_probe_arm(dfd_b0_plan* plan, int kind, int stage, int idx, int n) {
  if (!plan || n <= 0) { dfd::set_error("bad probe arguments", __FILE__, __LINE__); return -1; }
  std::lock_guard<std::mutex> lk(plan->mu);
  return dfd::probe_arm(plan->p, kind, stage, idx, n);
}
int dfd_b0_probe_read(dfd_b0_plan* plan, float* ms, int cap, int* count) {
  if (!plan || !ms || !count) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  std::lock_guard<std::mutex> lk(plan->mu);
  return dfd::probe_read(plan->p, ms, cap, count);
}
int dfd_b0_probe_disarm(dfd_b0_plan* plan) {
  if (!plan) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  std::lock_guard<std::mutex> lk(plan->mu);
  dfd::probe_disarm(plan->p);
  return 0;
}

int dfd_b0_saved_tensor(const dfd_b0_plan* plan, int idx, int64_t* off, int64_t* rows, int64_t* cols) {
  if (!plan || !off || !rows || !cols) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  const dfd::Plan& p = plan->p;
  const int64_t F = p.frames;
  struct E { int64_t o, r, c; };
  std::vector<E> v;
  v.push_back({p.o_ystem, F * p.H1 * p.W1, 32});
  for (const auto& b : p.blocks) {
    const int64_t Min = F * b.hin * b.win, Mout = F * b.hout * b.wout;
    if (!b.ds) v.push_back({b.o_y1, Min, b.mid});
    v.push_back({b.o_y2, Mout, b.mid});
    v.push_back({b.o_y3, Mout, b.cout});
    v.push_back({b.o_x, Mout, b.cout});
  }
  v.push_back({p.o_yh, F * p.Hf * p.Wf, 1280});
  if (idx < 0 || idx >= (int)v.size()) { dfd::set_error("saved tensor index out of range", __FILE__, __LINE__); return -1; }
  *off = v[idx].o; *rows = v[idx].r; *cols = v[idx].c;
  return 0;
}

int dfd_b0_grad_tensor(const dfd_b0_plan* plan, int block, int64_t* off, int64_t* rows, int64_t* cols) {
  if (!plan || !off || !rows || !cols) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  const dfd::Plan& p = plan->p;
  const int nb = (int)p.blocks.size();
  if (block < 1 || block > nb) { dfd::set_error("grad tensor: block out of range", __FILE__, __LINE__); return -1; }
  const int64_t F = p.frames;
  // backward_impl: block i writes the gradient of its input into o_gx[(i - 1) & 1]; the head
  // segment writes the gradient of the last block's output into o_gx[(nb - 1) & 1]
  *off = p.o_gx[(block - 1) & 1];
  if (block == nb) {
    *rows = F * p.Hf * p.Wf;
    *cols = p.head.cin;
  } else {
    const auto& b = p.blocks[block];
    *rows = F * b.hin * b.win;
    *cols = b.cin;
  }
  return 0;
}

int dfd_b0_fused_info(const dfd_b0_plan* plan, int* nblocks, int64_t* abort_offset) {
  if (!plan || !nblocks || !abort_offset) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  *nblocks = dfd::plan_fused7_blocks(plan->p);
  *abort_offset = plan->p.o_bar + 63 * 4;  // the int abort flag in the last word of the barrier region
  return 0;
}

int dfd_b0_plan_status(const dfd_b0_plan* plan, int* status) {
  if (!plan || !status) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  *status = dfd::plan_status(plan->p);
  return 0;
}

int dfd_b0_plan_clear_status(dfd_b0_plan* plan) {
  if (!plan) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  std::lock_guard<std::mutex> lk(plan->mu);
  if (plan->p.err_host) *reinterpret_cast<volatile int*>(plan->p.err_host) = 0;
  return 0;
}

int dfd_test_occupy(void* stream, int workgroups, int64_t microseconds) {
  DFD_GUARD_BEGIN
  return dfd::launch_occupy((hipStream_t)stream, workgroups, microseconds);
  DFD_GUARD_END
}

int dfd_test_group_sync(void* stream, int workgroups, int expected, double seconds, int* scratch, int* host_word) {
  DFD_GUARD_BEGIN
  return dfd::launch_group_sync_test((hipStream_t)stream, workgroups, expected, seconds, scratch, host_word);
  DFD_GUARD_END
}

int dfd_b0_segment_tensors(int seg, int* lo, int* hi) {
  if (seg < 0 || seg >= dfd::kNumSegments || !lo || !hi) {
    dfd::set_error("bad segment", __FILE__, __LINE__);
    return -1;
  }
  dfd::Plan dummy;
  dfd::plan_segment_range(dummy, seg, lo, hi);
  return 0;
}

// ---------------------------------------------------------------- head
static void head_layout(int B, int T, int D, int H, int F1, int64_t* offs, int64_t* total) {
  int64_t cur = 0;
  auto take = [&](int64_t n) { const int64_t o = cur; cur += (n + 63) & ~int64_t(63); return o; };
  offs[0] = take((int64_t)B * T * H);  // hid
  offs[1] = take((int64_t)B * T);      // e
  offs[2] = take((int64_t)B * D);      // g
  offs[3] = take((int64_t)B * F1);     // h1
  offs[4] = take((int64_t)B * F1);     // dh1
  offs[5] = take((int64_t)B * D);      // dg
  offs[6] = take((int64_t)B * T);      // dpe
  offs[7] = take((int64_t)B * T * H);  // dhid
  *total = cur;
}

static dfd::HeadWork head_work(float* w, int B, int T, int D, int H, int F1) {
  int64_t o[8], tot;
  head_layout(B, T, D, H, F1, o, &tot);
  return dfd::HeadWork{w + o[0], w + o[1], w + o[2], w + o[3], w + o[4], w + o[5], w + o[6], w + o[7]};
}

int64_t dfd_head_work_floats(int B, int T, int D, int H, int F1) {
  int64_t o[8], tot;
  head_layout(B, T, D, H, F1, o, &tot);
  return tot;
}

int dfd_head_forward(void* stream, int B, int T, int D, int H, int F1, int NC, int use_attn,
                     const float* const* p8, const float* features, float* work, uint64_t seed, float p,
                     float* logits, float* scores) {
  DFD_GUARD_BEGIN
  if (!p8 || !features || !work || !logits || !scores) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  dfd::HeadDims d{B, T, D, H, F1, NC, use_attn};
  dfd::HeadParams P{p8[0], p8[1], p8[2], p8[3], p8[4], p8[5], p8[6], p8[7]};
  dfd::HeadWork w = head_work(work, B, T, D, H, F1);
  return dfd::head_forward((hipStream_t)stream, d, P, features, w, seed, p, logits, scores);
  DFD_GUARD_END
}

int dfd_head_backward(void* stream, int B, int T, int D, int H, int F1, int NC, int use_attn,
                      const float* const* p8, const float* features, float* work, uint64_t seed, float p,
                      const float* scores, const float* dlogits, const float* dscores, float* dfeatures,
                      float* const* g8) {
  DFD_GUARD_BEGIN
  if (!p8 || !g8 || !features || !work || !dlogits || !dfeatures) {
    dfd::set_error("null argument", __FILE__, __LINE__);
    return -1;
  }
  dfd::HeadDims d{B, T, D, H, F1, NC, use_attn};
  dfd::HeadParams P{p8[0], p8[1], p8[2], p8[3], p8[4], p8[5], p8[6], p8[7]};
  dfd::HeadParams G{g8[0], g8[1], g8[2], g8[3], g8[4], g8[5], g8[6], g8[7]};
  dfd::HeadWork w = head_work(work, B, T, D, H, F1);
  return dfd::head_backward((hipStream_t)stream, d, P, features, w, seed, p, scores, dlogits, dscores, dfeatures, G);
  DFD_GUARD_END
}

int dfd_ce_forward(void* stream, const float* logits, const int64_t* labels, const float* weight, int B, int NC,
                   int64_t ignore_index, float* loss, float* wsum) {
  DFD_GUARD_BEGIN
  return dfd::ce_forward((hipStream_t)stream, logits, labels, weight, B, NC, ignore_index, loss, wsum);
  DFD_GUARD_END
}

int dfd_ce_backward(void* stream, const float* logits, const int64_t* labels, const float* weight, int B, int NC,
                    int64_t ignore_index, const float* wsum, const float* grad_out, float* dlogits) {
  DFD_GUARD_BEGIN
  return dfd::ce_backward((hipStream_t)stream, logits, labels, weight, B, NC, ignore_index, wsum, grad_out, dlogits);
  DFD_GUARD_END
}

static int loss_desc(dfd::LossDesc& d, int mode, int reduction, int B, int C, double gamma, double eps,
                     int64_t ignore_index) {
  if (!(eps >= 0.0 && eps < 1.0)) { dfd::set_error("classification loss: label_smoothing outside [0, 1)", __FILE__, __LINE__); return -1; }
  d.mode = mode; d.reduction = reduction; d.B = B; d.C = C;
  d.gamma = (float)gamma;
  d.q_on = (float)(1.0 - eps);
  d.q_off = mode == DFD_LOSS_FOCAL ? (C > 1 ? (float)(eps / (C - 1)) : 0.f) : (float)(eps / (C > 0 ? C : 1));
  d.ignore = ignore_index;
  return 0;
}

int64_t dfd_loss_work_floats(int B, int C) {
  return B < 1 || C < 1 || C > dfd::kLossMaxClasses ? -1 : dfd::loss_work_floats(B, C);
}

int dfd_loss_forward(void* stream, int mode, int reduction, const float* logits, const int64_t* labels,
                     const float* weight, int B, int C, double gamma, double label_smoothing, int64_t ignore_index,
                     float* work, float* loss) {
  DFD_GUARD_BEGIN
  if (!logits || !labels || !work || !loss) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  dfd::LossDesc d{};
  if (loss_desc(d, mode, reduction, B, C, gamma, label_smoothing, ignore_index) != 0) return -1;
  return dfd::loss_forward((hipStream_t)stream, d, logits, labels, weight, work, loss);
  DFD_GUARD_END
}

int dfd_loss_backward(void* stream, int mode, int reduction, const int64_t* labels, const float* weight, int B, int C,
                      double gamma, double label_smoothing, int64_t ignore_index, const float* work,
                      const float* grad_out, float* dlogits) {
  DFD_GUARD_BEGIN
  if (!labels || !work || !grad_out || !dlogits) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  dfd::LossDesc d{};
  if (loss_desc(d, mode, reduction, B, C, gamma, label_smoothing, ignore_index) != 0) return -1;
  return dfd::loss_backward((hipStream_t)stream, d, labels, weight, work, grad_out, dlogits);
  DFD_GUARD_END
}

int dfd_metrics_append(void* stream, const float* logits, const int64_t* labels, const float* loss, int B,
                       int64_t offset, int64_t capacity, float* probs, uint8_t* tags, double* loss_sums) {
  DFD_GUARD_BEGIN
  return dfd::metrics_append((hipStream_t)stream, logits, labels, loss, B, offset, capacity, probs, tags, loss_sums);
  DFD_GUARD_END
}

int dfd_metrics_finalize(void* stream, const float* probs, const uint8_t* tags, int64_t N, const float* thresholds,
                         int n_thresholds, int64_t* result) {
  DFD_GUARD_BEGIN
  return dfd::metrics_finalize((hipStream_t)stream, probs, tags, N, thresholds, n_thresholds, result);
  DFD_GUARD_END
}

int64_t dfd_ensemble_decide_floats(int M) {
  DFD_GUARD_BEGIN
  return dfd::ensemble_decide_floats(M);
  DFD_GUARD_END
}

int dfd_ensemble_decide(void* stream, const float* member_logits, const float* member_scores, const float* weights,
                        int M, int64_t V, int C, int T, int method, int fake_idx, float temperature, float* logits,
                        float* scores, float* block) {
  DFD_GUARD_BEGIN
  return dfd::ensemble_decide((hipStream_t)stream, member_logits, member_scores, weights, M, V, C, T, method, fake_idx,
                              temperature, logits, scores, block);
  DFD_GUARD_END
}

int dfd_grad_norm(void* stream, const float* grads, int64_t n, float max_norm, void* scratch, float* out2) {
  DFD_GUARD_BEGIN
  return dfd::grad_norm((hipStream_t)stream, grads, n, max_norm, (double*)scratch, 1024, out2);
  DFD_GUARD_END
}

int dfd_adam_step(void* stream, float* params, float* grads, float* m, float* v, int64_t n, double lr, double beta1,
                  double beta2, double eps, double weight_decay, int step, double grad_scale, int decoupled,
                  const float* clip_out2) {
  DFD_GUARD_BEGIN
  // scalars rounded exactly as torch.optim.{Adam,AdamW} (_single_tensor path) rounds them
  dfd::AdamHyper h{};
  h.omb1 = (float)(1.0 - beta1);
  h.beta2 = (float)beta2;
  h.omb2 = (float)(1.0 - beta2);
  h.eps = (float)eps;
  h.weight_decay = (float)weight_decay;
  h.decay = (float)(1.0 - lr * weight_decay);
  const double bc1 = 1.0 - std::pow(beta1, (double)step);
  const double bc2 = 1.0 - std::pow(beta2, (double)step);
  h.step_size = (float)(lr / bc1);
  h.bc2_sqrt = (float)std::sqrt(bc2);
  h.grad_scale = (float)grad_scale;
  h.decoupled = decoupled;
  return dfd::adam_step((hipStream_t)stream, params, grads, m, v, n, h, clip_out2);
  DFD_GUARD_END
}

int dfd_grad_norm_scaled(void* stream, const float* grads, int64_t n, float max_norm, float* scaler_state, void* scratch,
                         float* out2) {
  DFD_GUARD_BEGIN
  if (!scaler_state) { dfd::set_error("grad_norm_scaled: scaler state missing", __FILE__, __LINE__); return -1; }
  return dfd::grad_norm((hipStream_t)stream, grads, n, max_norm, (double*)scratch, 1024, out2, scaler_state);
  DFD_GUARD_END
}

int dfd_adam_step_scaled(void* stream, float* params, float* grads, float* m, float* v, int64_t n, double lr,
                         double beta1, double beta2, double eps, double weight_decay, double grad_scale, int decoupled,
                         const float* clip_out2, const float* scaler_state) {
  DFD_GUARD_BEGIN
  if (!scaler_state) { dfd::set_error("adam_step_scaled: scaler state missing", __FILE__, __LINE__); return -1; }
  dfd::AdamHyper h{};
  h.omb1 = (float)(1.0 - beta1);
  h.beta2 = (float)beta2;
  h.omb2 = (float)(1.0 - beta2);
  h.eps = (float)eps;
  h.weight_decay = (float)weight_decay;
  h.decay = (float)(1.0 - lr * weight_decay);
  h.grad_scale = (float)grad_scale;
  h.decoupled = decoupled;
  h.scaler = scaler_state;
  h.lr = lr;
  h.beta1d = beta1;
  h.beta2d = beta2;
  return dfd::adam_step((hipStream_t)stream, params, grads, m, v, n, h, clip_out2);
  DFD_GUARD_END
}

int dfd_loss_scale_update(void* stream, float* scaler_state, double growth_factor, double backoff_factor,
                          int growth_interval) {
  DFD_GUARD_BEGIN
  if (!scaler_state || growth_interval < 1) { dfd::set_error("loss_scale_update: bad arguments", __FILE__, __LINE__); return -1; }
  return dfd::loss_scale_update((hipStream_t)stream, scaler_state, (float)growth_factor, (float)backoff_factor,
                                growth_interval);
  DFD_GUARD_END
}

int dfd_collate_frames(void* stream, const uint8_t* src, const int64_t* sel, int64_t nsel, int64_t frame_bytes,
                       int out_f32, void* out) {
  DFD_GUARD_BEGIN
  if (nsel > 0 && (!src || !sel || !out)) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  return dfd::launch_collate_gather((hipStream_t)stream, src, sel, nsel, frame_bytes, out_f32 != 0, out);
  DFD_GUARD_END
}

// ---- augmentation / eval resize (k_augment.hip) ----
static bool aug_shape_ok(int n, int src_h, int src_w, int out_h, int out_w) {
  const int64_t lim = (int64_t)1 << 31;
  if (n < 0 || src_h < 1 || src_w < 1 || out_h < 1 || out_w < 1 || (int64_t)src_h * src_w * 3 >= lim ||
      (int64_t)std::max(out_h, 8) * std::max(out_w, 8) * 3 >= lim) {
    dfd::set_error("augment_frames: bad shape", __FILE__, __LINE__);
    return false;
  }
  if (n > 65535) { dfd::set_error("augment_frames: at most 65535 frames per call", __FILE__, __LINE__); return false; }
  return true;
}

// the rules of include/dfd_hip.h on one call's tables; nothing is enqueued for a table that fails them
static bool aug_table_ok(const int32_t* pi, const float* pf, int n, int src_h, int src_w, int out_h, int out_w) {
  char msg[160];
  for (int f = 0; f < n; ++f) {
    const int32_t* r = pi + (int64_t)f * DFD_AUG_PI;
    const float* q = pf + (int64_t)f * DFD_AUG_PF;
    const char* bad = nullptr;
    const int all = DFD_AUG_FLIP | DFD_AUG_JITTER | DFD_AUG_GRAY | DFD_AUG_DOWNUP | DFD_AUG_BLUR;
    int seen = 0;
    for (int o = 0; o < 4; ++o)
      if (r[5 + o] >= 0 && r[5 + o] < 4) seen |= 1 << r[5 + o];
    if (r[0] & ~all) bad = "unknown flag";
    else if (r[1] < 0 || r[2] < 0 || r[3] < 1 || r[4] < 1 || (int64_t)r[1] + r[3] > src_h || (int64_t)r[2] + r[4] > src_w)
      bad = "crop box outside the source";
    else if (seen != 15) bad = "jitter order is not a permutation of 0..3";
    else if (r[9] < 0 || r[9] > 255) bad = "hue shift outside 0..255";
    else if (r[10] < 1 || r[11] < 1 || r[10] > std::max(out_h, 8) || r[11] > std::max(out_w, 8))
      bad = "downscale size outside 1..max(out, 8)";
    else if ((r[0] & DFD_AUG_BLUR) && (out_h < 2 || out_w < 2)) bad = "blur needs an output of at least 2 x 2";
    else
      for (int k = 0; k < DFD_AUG_PF; ++k)
        if (!std::isfinite(q[k])) bad = "non-finite factor";
    if (bad) {
      snprintf(msg, sizeof(msg), "augment_frames: frame %d: %s", f, bad);
      dfd::set_error(msg, __FILE__, __LINE__);
      return false;
    }
  }
  return true;
}

int64_t dfd_augment_scratch_bytes(int n, int src_h, int src_w, int out_h, int out_w) {
  if (!aug_shape_ok(n, src_h, src_w, out_h, out_w)) return -1;
  return dfd::augment_scratch_bytes(n, src_h, src_w, out_h, out_w, false);
}

int64_t dfd_augment_jpeg_scratch_bytes(int n, int src_h, int src_w, int out_h, int out_w) {
  if (!aug_shape_ok(n, src_h, src_w, out_h, out_w)) return -1;
  return dfd::augment_scratch_bytes(n, src_h, src_w, out_h, out_w, true);
}

int dfd_augment_lds_resident(int src_h, int src_w, int out_h, int out_w) {
  if (!aug_shape_ok(1, src_h, src_w, out_h, out_w)) return -1;
  return dfd::augment_path(src_h, src_w, out_h, out_w);
}

int dfd_augment_frames(void* stream, const uint8_t* src, int n, int src_h, int src_w, const int32_t* params_i32,
                       const float* params_f32, int out_h, int out_w, uint8_t* out, void* scratch,
                       int64_t scratch_bytes) {
  DFD_GUARD_BEGIN
  if (!aug_shape_ok(n, src_h, src_w, out_h, out_w)) return -1;
  if (n == 0) return 0;
  if (!src || !params_i32 || !params_f32 || !out || !scratch) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  if (!aug_table_ok(params_i32, params_f32, n, src_h, src_w, out_h, out_w)) return -1;
  return dfd::launch_augment_frames((hipStream_t)stream, src, n, src_h, src_w, params_i32, params_f32, nullptr, out_h,
                                    out_w, out, scratch, scratch_bytes);
  DFD_GUARD_END
}

int dfd_augment_frames_jpeg(void* stream, const uint8_t* src, int n, int src_h, int src_w, const int32_t* params_i32,
                            const float* params_f32, const int32_t* quality, int out_h, int out_w, uint8_t* out,
                            void* scratch, int64_t scratch_bytes) {
  DFD_GUARD_BEGIN
  if (!aug_shape_ok(n, src_h, src_w, out_h, out_w)) return -1;
  if (n == 0) return 0;
  if (!src || !params_i32 || !params_f32 || !quality || !out || !scratch) {
    dfd::set_error("null argument", __FILE__, __LINE__);
    return -1;
  }
  if (!aug_table_ok(params_i32, params_f32, n, src_h, src_w, out_h, out_w)) return -1;
  for (int f = 0; f < n; ++f)
    if (quality[f] < 0 || quality[f] > 100) {
      char msg[160];
      snprintf(msg, sizeof(msg), "augment_frames: frame %d: JPEG quality %d outside 0..100", f, (int)quality[f]);
      dfd::set_error(msg, __FILE__, __LINE__);
      return -1;
    }
  return dfd::launch_augment_frames((hipStream_t)stream, src, n, src_h, src_w, params_i32, params_f32, quality, out_h,
                                    out_w, out, scratch, scratch_bytes);
  DFD_GUARD_END
}

// ---- ResNet-50 ensemble member (inference; k_resnet.hip + hipBLASLt) ----
int dfd_rn_im2col(void* stream, int dtype, const void* x, int N, int H, int W, int C, int kh, int kw, int stride,
                  int pad, int Kp, void* out) {
  DFD_GUARD_BEGIN
  if (!x || !out) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  if (dtype == 1)
    return dfd::launch_rn_im2col((hipStream_t)stream, (const dfd::bf16*)x, N, H, W, C, kh, kw, stride, pad, Kp,
                                 (dfd::bf16*)out);
  return dfd::launch_rn_im2col((hipStream_t)stream, (const float*)x, N, H, W, C, kh, kw, stride, pad, Kp, (float*)out);
  DFD_GUARD_END
}

int dfd_rn_stem_conv(void* stream, int dtype, const void* x, int input_fmt, const int64_t* strides4,
                     const float* norm6, int N, int H, int W, const void* w, const float* bias, void* out) {
  DFD_GUARD_BEGIN
  if (!x || !out || !strides4 || !w || !bias) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  if (dtype != 1) { dfd::set_error("rn stem conv: bf16 only (fp32: dfd_rn_stem_im2col + dfd_rn_gemm)", __FILE__, __LINE__); return -1; }
  dfd::InputFmt in{};
  in.u8 = input_fmt == DFD_INPUT_U8 ? 1 : 0;
  for (int c = 0; c < 3; ++c) {
    in.mean[c] = norm6 ? norm6[c] : 0.f;
    in.stdv[c] = norm6 ? norm6[3 + c] : 1.f;
  }
  return dfd::launch_rn_stem_conv((hipStream_t)stream, x, in, strides4, N, H, W, (const dfd::bf16*)w, bias,
                                  (dfd::bf16*)out);
  DFD_GUARD_END
}

int dfd_rn_stem_im2col(void* stream, int dtype, const void* x, int input_fmt, const int64_t* strides4,
                       const float* norm6, int N, int H, int W, void* out) {
  DFD_GUARD_BEGIN
  if (!x || !out || !strides4) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  dfd::InputFmt in{};
  in.u8 = input_fmt == DFD_INPUT_U8 ? 1 : 0;
  for (int c = 0; c < 3; ++c) {
    in.mean[c] = norm6 ? norm6[c] : 0.f;
    in.stdv[c] = norm6 ? norm6[3 + c] : 1.f;
  }
  if (dtype == 1) return dfd::launch_rn_stem_im2col((hipStream_t)stream, x, in, strides4, N, H, W, (dfd::bf16*)out);
  return dfd::launch_rn_stem_im2col((hipStream_t)stream, x, in, strides4, N, H, W, (float*)out);
  DFD_GUARD_END
}

int dfd_rn_gemm(void* stream, int dtype, const void* A, const void* B, void* C, const void* R, const float* bias,
                int relu, int64_t M, int N, int K) {
  DFD_GUARD_BEGIN
  if (!A || !B || !C || !bias) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  dfd::RnConvGeom g{};
  g.KH = g.KW = g.stride = 1;
  if (dtype == 1)
    return dfd::launch_rn_conv((hipStream_t)stream, (const dfd::bf16*)A, (const dfd::bf16*)B, (dfd::bf16*)C,
                               (const dfd::bf16*)R, bias, relu, g, M, N, K);
  return dfd::launch_rn_conv((hipStream_t)stream, (const float*)A, (const float*)B, (float*)C, (const float*)R, bias,
                             relu, g, M, N, K);
  DFD_GUARD_END
}

int dfd_rn_conv(void* stream, int dtype, const void* x, int N, int H, int W, int Cin, int kh, int kw, int stride,
                int pad, const void* w, const float* bias, const void* res, int relu, int Cout, void* out) {
  DFD_GUARD_BEGIN
  if (!x || !w || !bias || !out) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || kh <= 0 || kw <= 0 || stride <= 0 || pad < 0 || Cout <= 0) {
    dfd::set_error("rn_conv: bad shape", __FILE__, __LINE__);
    return -1;
  }
  dfd::RnConvGeom g{N, H, W, Cin, kh, kw, stride, pad, (H + 2 * pad - kh) / stride + 1,
                    (W + 2 * pad - kw) / stride + 1, 0};
  while ((1 << g.cin_log2) < Cin && g.cin_log2 < 30) ++g.cin_log2;
  if (g.Ho <= 0 || g.Wo <= 0) { dfd::set_error("rn_conv: empty output", __FILE__, __LINE__); return -1; }
  const int64_t M = (int64_t)N * g.Ho * g.Wo;
  const int K = kh * kw * Cin;
  if (dtype == 1)
    return dfd::launch_rn_conv((hipStream_t)stream, (const dfd::bf16*)x, (const dfd::bf16*)w, (dfd::bf16*)out,
                               (const dfd::bf16*)res, bias, relu, g, M, Cout, K);
  return dfd::launch_rn_conv((hipStream_t)stream, (const float*)x, (const float*)w, (float*)out, (const float*)res,
                             bias, relu, g, M, Cout, K);
  DFD_GUARD_END
}

int dfd_rn_maxpool(void* stream, int dtype, const void* x, int N, int H, int W, int C, void* out) {
  DFD_GUARD_BEGIN
  if (!x || !out) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  if (dtype == 1)
    return dfd::launch_rn_maxpool((hipStream_t)stream, (const dfd::bf16*)x, N, H, W, C, (dfd::bf16*)out);
  return dfd::launch_rn_maxpool((hipStream_t)stream, (const float*)x, N, H, W, C, (float*)out);
  DFD_GUARD_END
}

int dfd_rn_avgpool(void* stream, int dtype, const void* x, int N, int HW, int C, float* out) {
  DFD_GUARD_BEGIN
  if (!x || !out) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  if (dtype == 1) return dfd::launch_rn_avgpool((hipStream_t)stream, (const dfd::bf16*)x, N, HW, C, out);
  return dfd::launch_rn_avgpool((hipStream_t)stream, (const float*)x, N, HW, C, out);
  DFD_GUARD_END
}

// ---- ResNet-50 training (fp32)
// the ResNet-50 training convolutions sum K in two levels (k_conv.hip FOLD): its train-mode BN
// chain needs the accuracy (tests/test_resnet_train_gpu.py holds it to torch fp32's distance to fp64)
static dfd::ConvGeom rn_geom(int N, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad) {
  return dfd::ConvGeom{N, H, W, Cin, Cout, kh, kw, stride, pad, (H + 2 * pad - kh) / stride + 1,
                       (W + 2 * pad - kw) / stride + 1, true};
}

int64_t dfd_rn_conv_stat_rows(int N, int Ho, int Wo) { return ((int64_t)N * Ho * Wo + 63) / 64; }

int dfd_rn_train_conv_fwd(void* stream, const float* x, const int64_t* xs4, int N, int H, int W, int Cin,
                          const float* w, int Cout, int kh, int kw, int stride, int pad, float* wpack, float* y,
                          float* stats) {
  DFD_GUARD_BEGIN
  if (!x || !xs4 || !w || !wpack || !y || !stats) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  const dfd::ConvGeom g = rn_geom(N, H, W, Cin, Cout, kh, kw, stride, pad);
  if ((int64_t)N * g.Ho * g.Wo >= (1ll << 31)) { dfd::set_error("rn conv: too many rows", __FILE__, __LINE__); return -1; }
  const int64_t xs[4] = {xs4[0], xs4[1], xs4[2], xs4[3]};
  int rows = 0;
  return dfd::conv_forward((hipStream_t)stream, g, x, xs, w, nullptr, wpack, y, stats, &rows);
  DFD_GUARD_END
}

int dfd_rn_bn_train_finalize(void* stream, const float* stats, int rows, int64_t count, int C, const float* gamma,
                             const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                             float* mean, float* invstd, float* scale, float* shift) {
  DFD_GUARD_BEGIN
  if (!stats || !gamma || !beta || !mean || !invstd || !scale || !shift) {
    dfd::set_error("null argument", __FILE__, __LINE__);
    return -1;
  }
  return dfd::launch_bn_finalize((hipStream_t)stream, stats, rows, count, C, gamma, beta, running_mean, running_var,
                                 momentum, eps, true, mean, invstd, scale, shift, dfd::kConvStatRows);
  DFD_GUARD_END
}

int dfd_rn_bn_act(void* stream, const float* y, const float* mean, const float* scale, const float* beta,
                  const float* res, int relu, int64_t M, int C, float* out) {
  DFD_GUARD_BEGIN
  if (!y || !mean || !scale || !beta || !out) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  return dfd::rn_bn_act((hipStream_t)stream, y, mean, scale, beta, res, relu, M, C, out);
  DFD_GUARD_END
}

int dfd_rn_pool_train_fwd(void* stream, const float* y, const float* mean, const float* scale, const float* beta,
                          int N, int H, int W, int C, float* out, uint8_t* argmax) {
  DFD_GUARD_BEGIN
  if (!y || !mean || !scale || !beta || !out || !argmax) {
    dfd::set_error("null argument", __FILE__, __LINE__);
    return -1;
  }
  return dfd::bn_relu_pool_fwd((hipStream_t)stream, y, mean, scale, beta, N, H, W, C, (H + 2 - 3) / 2 + 1,
                               (W + 2 - 3) / 2 + 1, out, argmax);
  DFD_GUARD_END
}

int dfd_rn_pool_train_bwd(void* stream, const float* dout, const uint8_t* argmax, const float* y, const float* mean,
                          const float* scale, const float* beta, int N, int H, int W, int C, float* g) {
  DFD_GUARD_BEGIN
  if (!dout || !argmax || !y || !mean || !scale || !beta || !g) {
    dfd::set_error("null argument", __FILE__, __LINE__);
    return -1;
  }
  return dfd::bn_relu_pool_bwd((hipStream_t)stream, dout, argmax, y, mean, scale, beta, N, H, W, C, (H + 2 - 3) / 2 + 1,
                               (W + 2 - 3) / 2 + 1, g);
  DFD_GUARD_END
}

int dfd_rn_relu_bwd(void* stream, const float* dout, const float* out, int64_t n, float* g) {
  DFD_GUARD_BEGIN
  if (!dout || !out || !g) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  return dfd::rn_relu_bwd((hipStream_t)stream, dout, out, n, g);
  DFD_GUARD_END
}

int dfd_rn_gap_bwd(void* stream, const float* dfeat, const float* out, int N, int HW, int C, float* g) {
  DFD_GUARD_BEGIN
  if (!dfeat || !out || !g) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  return dfd::rn_gap_bwd((hipStream_t)stream, dfeat, out, N, HW, C, g);
  DFD_GUARD_END
}

int dfd_rn_bn_train_bwd(void* stream, const float* g, const float* y, int64_t M, int C, const float* mean,
                        const float* invstd, const float* scale, const float* shift, const float* gamma, float* dgamma,
                        float* dbeta, float* stats, float* coef, float* dy) {
  DFD_GUARD_BEGIN
  if (!g || !y || !mean || !invstd || !scale || !shift || !gamma || !dgamma || !dbeta || !stats || !coef || !dy) {
    dfd::set_error("null argument", __FILE__, __LINE__);
    return -1;
  }
  return dfd::rn_bn_train_bwd((hipStream_t)stream, g, y, M, C, mean, invstd, scale, shift, gamma, dgamma, dbeta,
                              stats, coef, dy);
  DFD_GUARD_END
}

int dfd_rn_bn_train_bwd_relu(void* stream, const float* da, const float* relu_out, const float* y, int64_t M, int C,
                             const float* mean, const float* invstd, const float* gamma, float* dgamma, float* dbeta,
                             float* stats, float* coef, float* dy) {
  DFD_GUARD_BEGIN
  if (!da || !relu_out || !y || !mean || !invstd || !gamma || !dgamma || !dbeta || !stats || !coef || !dy) {
    dfd::set_error("null argument", __FILE__, __LINE__);
    return -1;
  }
  return dfd::rn_bn_train_bwd_relu((hipStream_t)stream, da, relu_out, y, M, C, mean, invstd, gamma, dgamma, dbeta,
                                   stats, coef, dy);
  DFD_GUARD_END
}

int dfd_rn_conv_dgrad(void* stream, const float* dy, int N, int H, int W, int Cin, const float* w, int Cout, int kh,
                      int kw, int stride, int pad, float* wpack, float* wpack_t, float* dx) {
  DFD_GUARD_BEGIN
  if (!dy || !w || !wpack || !wpack_t || !dx) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  const dfd::ConvGeom g = rn_geom(N, H, W, Cin, Cout, kh, kw, stride, pad);
  return dfd::conv_dgrad((hipStream_t)stream, g, dy, w, wpack, wpack_t, dx);
  DFD_GUARD_END
}

int dfd_rn_conv_dgrad_res(void* stream, const float* dy, int N, int H, int W, int Cin, const float* w, int Cout, int kh,
                          int kw, int stride, int pad, float* wpack, float* wpack_t, const float* res, float* dx) {
  DFD_GUARD_BEGIN
  if (!dy || !w || !wpack || !wpack_t || !res || !dx) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  const dfd::ConvGeom g = rn_geom(N, H, W, Cin, Cout, kh, kw, stride, pad);
  return dfd::conv_dgrad((hipStream_t)stream, g, dy, w, wpack, wpack_t, dx, res);
  DFD_GUARD_END
}

int64_t dfd_rn_conv_wgrad_slab_floats(int N, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad) {
  return dfd::conv_wgrad_slab_floats(rn_geom(N, H, W, Cin, Cout, kh, kw, stride, pad));
}

int dfd_rn_conv_wgrad(void* stream, const float* x, const int64_t* xs4, int N, int H, int W, int Cin, const float* dy,
                      int Cout, int kh, int kw, int stride, int pad, float* slab, int64_t slab_floats, float* dw) {
  DFD_GUARD_BEGIN
  if (!x || !xs4 || !dy || !slab || !dw) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  const dfd::ConvGeom g = rn_geom(N, H, W, Cin, Cout, kh, kw, stride, pad);
  if ((int64_t)Cout * Cin * kh * kw > slab_floats) { dfd::set_error("rn wgrad: slab too small", __FILE__, __LINE__); return -1; }
  const int64_t xs[4] = {xs4[0], xs4[1], xs4[2], xs4[3]};
  return dfd::conv_wgrad((hipStream_t)stream, g, x, xs, dy, slab, slab_floats, dw);
  DFD_GUARD_END
}

// ---- test seam: the three convolution launchers with a caller-given fold flag and an optional bias
// (tests/test_conv_kernels_gpu.py; fold = 0 with a bias are CNNLSTMHybrid's templates, which the
// dfd_rn_* entry points above never reach).  Product paths do not call these.
static dfd::ConvGeom test_geom(int N, int H, int W, int Cin, int Cout, int kh, int kw, int stride, int pad, int fold) {
  dfd::ConvGeom g = rn_geom(N, H, W, Cin, Cout, kh, kw, stride, pad);
  g.fold = fold != 0;
  return g;
}

int dfd_test_conv_fwd(void* stream, const float* x, const int64_t* xs4, int N, int H, int W, int Cin, const float* w,
                      const float* bias, int Cout, int kh, int kw, int stride, int pad, int fold, float* wpack, float* y,
                      float* stats) {
  DFD_GUARD_BEGIN
  if (!x || !xs4 || !w || !wpack || !y || !stats) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  const dfd::ConvGeom g = test_geom(N, H, W, Cin, Cout, kh, kw, stride, pad, fold);
  if ((int64_t)N * g.Ho * g.Wo >= (1ll << 31)) { dfd::set_error("test conv: too many rows", __FILE__, __LINE__); return -1; }
  const int64_t xs[4] = {xs4[0], xs4[1], xs4[2], xs4[3]};
  int rows = 0;
  return dfd::conv_forward((hipStream_t)stream, g, x, xs, w, bias, wpack, y, stats, &rows);
  DFD_GUARD_END
}

int dfd_test_conv_dgrad(void* stream, const float* dy, int N, int H, int W, int Cin, const float* w, int Cout, int kh,
                        int kw, int stride, int pad, int fold, float* wpack, float* wpack_t, float* dx) {
  DFD_GUARD_BEGIN
  if (!dy || !w || !wpack || !wpack_t || !dx) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  if ((int64_t)N * H * W >= (1ll << 31)) { dfd::set_error("test conv: too many rows", __FILE__, __LINE__); return -1; }
  const dfd::ConvGeom g = test_geom(N, H, W, Cin, Cout, kh, kw, stride, pad, fold);
  return dfd::conv_dgrad((hipStream_t)stream, g, dy, w, wpack, wpack_t, dx);
  DFD_GUARD_END
}

int dfd_test_conv_wgrad(void* stream, const float* x, const int64_t* xs4, int N, int H, int W, int Cin, const float* dy,
                        int Cout, int kh, int kw, int stride, int pad, int fold, float* slab, int64_t slab_floats,
                        float* dw) {
  DFD_GUARD_BEGIN
  if (!x || !xs4 || !dy || !slab || !dw) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  const dfd::ConvGeom g = test_geom(N, H, W, Cin, Cout, kh, kw, stride, pad, fold);
  if ((int64_t)N * g.Ho * g.Wo >= (1ll << 31)) { dfd::set_error("test conv: too many rows", __FILE__, __LINE__); return -1; }
  if ((int64_t)Cout * Cin * kh * kw > slab_floats) { dfd::set_error("test wgrad: slab too small", __FILE__, __LINE__); return -1; }
  const int64_t xs[4] = {xs4[0], xs4[1], xs4[2], xs4[3]};
  return dfd::conv_wgrad((hipStream_t)stream, g, x, xs, dy, slab, slab_floats, dw);
  DFD_GUARD_END
}

// ---- test seam: the launchers of k_vit.hip one by one (tests/test_vit_kernels_gpu.py).  dtype 0 = fp32, 1 = bf16
// storage; thin calls of the launch_* functions vit.cpp uses.  Product paths do not call these.
#define VIT_T(dtype, CALL)                                                                     \
  do {                                                                                         \
    if ((dtype) == 0) { using T = float; return CALL; }                                        \
    if ((dtype) == 1) { using T = dfd::bf16; return CALL; }                                    \
    dfd::set_error("test vit: dtype must be 0 (fp32) or 1 (bf16)", __FILE__, __LINE__);        \
    return -1;                                                                                 \
  } while (0)

static dfd::BgOp test_bgop(const int64_t* o) { return dfd::BgOp{o[0], (int)o[1], o[2], o[3]}; }

int dfd_test_vit_bgemm(void* stream, int dtype, int ta, int tb, int batch, int M, int N, int K, float alpha,
                       const void* A, const int64_t* a4, const void* B, const int64_t* b4, void* C, const int64_t* c4) {
  DFD_GUARD_BEGIN
  if (!A || !a4 || !B || !b4 || !C || !c4 || a4[1] < 1 || b4[1] < 1 || c4[1] < 1) {
    dfd::set_error("test bgemm: null argument or inner < 1", __FILE__, __LINE__);
    return -1;
  }
  VIT_T(dtype, dfd::launch_bgemm<T>((hipStream_t)stream, ta != 0, tb != 0, batch, M, N, K, alpha, (const T*)A,
                                    test_bgop(a4), (const T*)B, test_bgop(b4), (T*)C, test_bgop(c4)));
  DFD_GUARD_END
}

int dfd_test_vit_softmax_fwd(void* stream, int dtype, const void* S, void* P, int64_t rows, int n, int ld) {
  DFD_GUARD_BEGIN
  if (!S || !P || rows < 1 || n < 1 || n > ld) { dfd::set_error("test softmax: bad argument", __FILE__, __LINE__); return -1; }
  VIT_T(dtype, dfd::launch_softmax_fwd<T>((hipStream_t)stream, (const T*)S, (T*)P, rows, n, ld));
  DFD_GUARD_END
}

int dfd_test_vit_softmax_bwd(void* stream, int dtype, const void* P, const void* dP, void* dS, int64_t rows, int n,
                             int ld, float scale) {
  DFD_GUARD_BEGIN
  if (!P || !dP || !dS || rows < 1 || n < 1 || n > ld || ld > 64 * dfd::VIT_SM_PER_LANE) {
    dfd::set_error("test softmax: bad argument", __FILE__, __LINE__);
    return -1;
  }
  VIT_T(dtype, dfd::launch_softmax_bwd<T>((hipStream_t)stream, (const T*)P, (const T*)dP, (T*)dS, rows, n, ld, scale));
  DFD_GUARD_END
}

int dfd_test_vit_ln_fwd(void* stream, int dtype, int out_f32, const void* X, int64_t ldx, const float* g,
                        const float* b, void* Y, int64_t ldy, float* mean, float* rstd, int64_t rows, int C, float eps) {
  DFD_GUARD_BEGIN
  if (!X || !g || !b || !Y || !mean || !rstd || rows < 1 || ldx < C || ldy < C) {
    dfd::set_error("test layernorm: bad argument", __FILE__, __LINE__);
    return -1;
  }
  hipStream_t s = (hipStream_t)stream;
  if (dtype == 1 && out_f32)
    return dfd::launch_ln_fwd<dfd::bf16, float>(s, (const dfd::bf16*)X, ldx, g, b, (float*)Y, ldy, mean, rstd, rows, C, eps);
  VIT_T(dtype, (dfd::launch_ln_fwd<T, T>(s, (const T*)X, ldx, g, b, (T*)Y, ldy, mean, rstd, rows, C, eps)));
  DFD_GUARD_END
}

int dfd_test_vit_ln_bwd(void* stream, int dtype, int dy_f32, const void* X, int64_t ldx, const void* dY, int64_t ldd,
                        const float* g, const float* mean, const float* rstd, const void* dres, void* dX, int64_t rows,
                        int C, float* part, int64_t part_cap, float* dgamma, float* dbeta, int accumulate) {
  DFD_GUARD_BEGIN
  if (!X || !dY || !g || !mean || !rstd || !dX || !part || !dgamma || !dbeta || rows < 1 || ldx < C || ldd < C ||
      part_cap < 2LL * C) {
    dfd::set_error("test layernorm: bad argument", __FILE__, __LINE__);
    return -1;
  }
  hipStream_t s = (hipStream_t)stream;
  if (dtype == 1 && dy_f32)
    return dfd::launch_ln_bwd<dfd::bf16, float>(s, (const dfd::bf16*)X, ldx, (const float*)dY, ldd, g, mean, rstd,
                                                (const dfd::bf16*)dres, (dfd::bf16*)dX, rows, C, part, part_cap, dgamma,
                                                dbeta, accumulate != 0);
  VIT_T(dtype, (dfd::launch_ln_bwd<T, T>(s, (const T*)X, ldx, (const T*)dY, ldd, g, mean, rstd, (const T*)dres, (T*)dX,
                                         rows, C, part, part_cap, dgamma, dbeta, accumulate != 0)));
  DFD_GUARD_END
}

int dfd_test_vit_patch_gather(void* stream, int dtype, const float* x, const int64_t* x_strides5, int nodes, int H,
                              int W, int images, void* A) {
  DFD_GUARD_BEGIN
  if (!x || !x_strides5 || !A || nodes < 1 || images < 1 || images % nodes) {
    dfd::set_error("test patch gather: bad argument", __FILE__, __LINE__);
    return -1;
  }
  const dfd::VitImg im{nodes, H, W, x_strides5[0], x_strides5[1], x_strides5[2], x_strides5[3], x_strides5[4]};
  VIT_T(dtype, dfd::launch_patch_gather<T>((hipStream_t)stream, x, im, images, (T*)A));
  DFD_GUARD_END
}

int dfd_test_vit_tokens_fwd(void* stream, int dtype, const void* PE, const float* cls, const float* pos, int images,
                            int ntok, int D, void* X0) {
  DFD_GUARD_BEGIN
  if (!PE || !cls || !pos || !X0 || images < 1 || ntok < 2 || D < 8 || D % 8) {
    dfd::set_error("test tokens: bad argument", __FILE__, __LINE__);
    return -1;
  }
  VIT_T(dtype, dfd::launch_tokens_fwd<T>((hipStream_t)stream, (const T*)PE, cls, pos, images, ntok, D, (T*)X0));
  DFD_GUARD_END
}

int dfd_test_vit_tokens_bwd(void* stream, int dtype, const void* dX0, int images, int ntok, int D, void* dPE,
                            float* dpos, float* dcls) {
  DFD_GUARD_BEGIN
  if (!dX0 || !dPE || !dpos || !dcls || images < 1 || ntok < 2 || D < 1) {
    dfd::set_error("test tokens: bad argument", __FILE__, __LINE__);
    return -1;
  }
  VIT_T(dtype, dfd::launch_tokens_bwd<T>((hipStream_t)stream, (const T*)dX0, images, ntok, D, (T*)dPE, dpos, dcls));
  DFD_GUARD_END
}

int dfd_test_vit_wcast(void* stream, int dtype, int nseg, const float* const* src, void* const* dst,
                       void* const* dst_t, const int* rows, const int* cols) {
  DFD_GUARD_BEGIN
  if (!src || !dst || !dst_t || !rows || !cols || nseg < 1 || nseg > 8) {
    dfd::set_error("test wcast: bad argument", __FILE__, __LINE__);
    return -1;
  }
  dfd::VitCast cs{};
  for (int i = 0; i < nseg; ++i) {
    if (!src[i] || rows[i] < 1 || cols[i] < 1) { dfd::set_error("test wcast: bad segment", __FILE__, __LINE__); return -1; }
    cs.seg[i] = {src[i], dst[i], dst_t[i], rows[i], cols[i]};
  }
  VIT_T(dtype, dfd::launch_wcast<T>((hipStream_t)stream, cs, nseg));
  DFD_GUARD_END
}

int dfd_test_vit_colsum(void* stream, int dtype, const void* X, int64_t M, int N, float* part, int64_t part_cap,
                        float* out, int accumulate) {
  DFD_GUARD_BEGIN
  if (!X || !part || !out || M < 1 || N < 8 || part_cap < N) {
    dfd::set_error("test colsum: bad argument", __FILE__, __LINE__);
    return -1;
  }
  VIT_T(dtype, dfd::launch_colsum<T>((hipStream_t)stream, (const T*)X, M, N, part, part_cap, out, accumulate != 0));
  DFD_GUARD_END
}

int dfd_test_vit_gelu(void* stream, void* Z, void* out, int64_t n, int mode) {
  DFD_GUARD_BEGIN
  if (!Z || !out) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  return dfd::launch_gelu((hipStream_t)stream, (dfd::bf16*)Z, (dfd::bf16*)out, n, mode);
  DFD_GUARD_END
}
#undef VIT_T

// ---- ResNet-50 training (bf16, k_rn16.hip)
int dfd_rn16_pack_weights(void* stream, const float* w, int Cout, int Cin, int k, void* wf, void* wd) {
  DFD_GUARD_BEGIN
  if (!w || !wf) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  return dfd::rn16_pack_weights((hipStream_t)stream, w, Cout, Cin, k * k, (dfd::bf16*)wf, (dfd::bf16*)wd);
  DFD_GUARD_END
}

int dfd_rn16_pack_all(void* stream, const int64_t* table, int n, int64_t max_elems, void* out) {
  DFD_GUARD_BEGIN
  if (!table || !out) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  return dfd::rn16_pack_all((hipStream_t)stream, table, n, max_elems, (dfd::bf16*)out);
  DFD_GUARD_END
}

int dfd_rn16_conv_fwd(void* stream, const void* x, int N, int H, int W, int Cin, const void* wf, int Cout, int k,
                      int stride, int pad, void* y, float* stats, int* stat_rows) {
  DFD_GUARD_BEGIN
  if (!x || !wf || !y || !stats || !stat_rows) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  return dfd::rn16_conv_fwd((hipStream_t)stream, (const dfd::bf16*)x, N, H, W, Cin, (const dfd::bf16*)wf, Cout, k, stride,
                            pad, (dfd::bf16*)y, stats, stat_rows);
  DFD_GUARD_END
}

int dfd_rn16_conv_dgrad(void* stream, const void* dy, int N, int H, int W, int Cin, const void* wd, int Cout, int k,
                        int stride, int pad, const void* res, void* dx) {
  DFD_GUARD_BEGIN
  if (!dy || !wd || !dx) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  return dfd::rn16_conv_dgrad((hipStream_t)stream, (const dfd::bf16*)dy, N, H, W, Cin, (const dfd::bf16*)wd, Cout, k,
                              stride, pad, (const dfd::bf16*)res, (dfd::bf16*)dx);
  DFD_GUARD_END
}

int64_t dfd_rn16_conv_wgrad_slab_floats(int N, int H, int W, int Cin, int Cout, int k, int stride, int pad) {
  return dfd::rn16_conv_wgrad_slab_floats(N, H, W, Cin, Cout, k, stride, pad);
}

int dfd_rn16_conv_wgrad(void* stream, const void* x, int N, int H, int W, int Cin, const void* dy, int Cout, int k,
                        int stride, int pad, float* slab, int64_t slab_floats, float* dw) {
  DFD_GUARD_BEGIN
  if (!x || !dy || !slab || !dw) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  return dfd::rn16_conv_wgrad((hipStream_t)stream, (const dfd::bf16*)x, N, H, W, Cin, (const dfd::bf16*)dy, Cout, k,
                              stride, pad, slab, slab_floats, dw);
  DFD_GUARD_END
}

int dfd_rn16_bn_act(void* stream, const void* y, const float* mean, const float* scale, const float* beta,
                    const void* res, int relu, int64_t M, int C, void* out) {
  DFD_GUARD_BEGIN
  if (!y || !mean || !scale || !beta || !out) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  return dfd::rn16_bn_act((hipStream_t)stream, (const dfd::bf16*)y, mean, scale, beta, (const dfd::bf16*)res, relu, M,
                          C, (dfd::bf16*)out);
  DFD_GUARD_END
}

int dfd_rn16_relu_bwd(void* stream, const void* dout, const void* out, int64_t n, void* g) {
  DFD_GUARD_BEGIN
  if (!dout || !out || !g) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  return dfd::rn16_relu_bwd((hipStream_t)stream, (const dfd::bf16*)dout, (const dfd::bf16*)out, n, (dfd::bf16*)g);
  DFD_GUARD_END
}

int dfd_rn16_gap_bwd(void* stream, const float* dfeat, const void* out, int N, int HW, int C, void* g) {
  DFD_GUARD_BEGIN
  if (!dfeat || !out || !g) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  return dfd::rn16_gap_bwd((hipStream_t)stream, dfeat, (const dfd::bf16*)out, N, HW, C, (dfd::bf16*)g);
  DFD_GUARD_END
}

int dfd_rn16_cast(void* stream, const void* src, int to_bf16, int64_t n, void* dst) {
  DFD_GUARD_BEGIN
  if (!src || !dst) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  return dfd::rn16_cast((hipStream_t)stream, src, to_bf16, n, dst);
  DFD_GUARD_END
}

int dfd_rn16_bn_finalize(void* stream, const float* stats, int rows, int64_t count, int C, const float* gamma,
                         const float* beta, float* running_mean, float* running_var, float momentum, float eps,
                         float* mean, float* invstd, float* scale, float* shift) {
  DFD_GUARD_BEGIN
  if (!stats || !gamma || !beta || !running_mean || !running_var || !mean || !invstd || !scale || !shift) {
    dfd::set_error("null argument", __FILE__, __LINE__);
    return -1;
  }
  return dfd::launch_bn_finalize((hipStream_t)stream, stats, rows, count, C, gamma, beta, running_mean, running_var,
                                 momentum, eps, true, mean, invstd, scale, shift);
  DFD_GUARD_END
}

int dfd_rn16_bn_train_bwd(void* stream, const void* g, const void* relu_out, const void* y, int64_t M, int C,
                          const float* mean, const float* invstd, const float* scale, const float* shift,
                          const float* gamma, float* dgamma, float* dbeta, float* stats, float* coef, void* dy) {
  DFD_GUARD_BEGIN
  if (!g || !y || !mean || !invstd || !scale || !shift || !gamma || !dgamma || !dbeta || !stats || !coef || !dy) {
    dfd::set_error("null argument", __FILE__, __LINE__);
    return -1;
  }
  return dfd::rn16_bn_train_bwd((hipStream_t)stream, (const dfd::bf16*)g, (const dfd::bf16*)relu_out,
                                (const dfd::bf16*)y, M, C, mean, invstd, scale, shift, gamma, dgamma, dbeta, stats,
                                coef, (dfd::bf16*)dy);
  DFD_GUARD_END
}

// the kernel test seams' overrides (dfd_set_tuning): read only by dfd_pw_conv / dfd_pw_conv_wgrad /
// dfd_vgemm, which install a snapshot for their own launch; plans and models never see them
static std::mutex g_seam_mu;
static dfd::Tuning g_seam;
static dfd::Tuning seam_snapshot() {
  std::lock_guard<std::mutex> lk(g_seam_mu);
  return g_seam;
}

int64_t dfd_set_tuning(const char* key, int64_t value) {
  if (key && strcmp(key, "rnn_step") == 0) return dfd::set_rnn_step(value);
  for (int k = 0; key && k < dfd::TK_COUNT; ++k)
    if (strcmp(key, dfd::kTuneNames[k]) == 0) {
      std::lock_guard<std::mutex> lk(g_seam_mu);
      const int64_t prev = g_seam.v[k] == dfd::kTuneUnset ? dfd::kTuneDefault[k] : g_seam.v[k];
      g_seam.v[k] = value;
      return prev;
    }
  dfd::set_error("set_tuning: unknown key", __FILE__, __LINE__);
  return -1;
}

static bool pw_args_ok(int dtype, int64_t M, int N, int K, int pro_mode, const float* scale, const float* shift,
                       const float* gate, int rows_per_frame) {
  if (dtype != DFD_DTYPE_F32 && dtype != DFD_DTYPE_BF16 && dtype != DFD_DTYPE_F16) {
    dfd::set_error("pw: bad dtype", __FILE__, __LINE__);
    return false;
  }
  if (M < 0 || N <= 0 || K <= 0) { dfd::set_error("pw: bad shape", __FILE__, __LINE__); return false; }
  if (pro_mode != dfd::PRO_NONE && pro_mode != dfd::PRO_BN_SILU && pro_mode != dfd::PRO_BN_SILU_G &&
      pro_mode != dfd::PRO_GATE) {
    dfd::set_error("pw: bad prologue mode", __FILE__, __LINE__);
    return false;
  }
  if (dfd::pro_is_bn(pro_mode) && (!scale || !shift)) { dfd::set_error("pw: scale/shift missing", __FILE__, __LINE__); return false; }
  if (dfd::pro_is_gated(pro_mode) && (!gate || rows_per_frame <= 0)) {
    dfd::set_error("pw: gate / rows_per_frame missing", __FILE__, __LINE__);
    return false;
  }
  return true;
}

int dfd_pw_conv(void* stream, int dtype, const void* A, const void* W, void* C, const void* R, int64_t M, int N, int K,
                int pro_mode, const float* scale, const float* shift, const float* gate, int rows_per_frame,
                float* stats, int* stat_rows) {
  DFD_GUARD_BEGIN
  const dfd::Tuning tn = seam_snapshot();
  const dfd::TuningScope ts(&tn);
  if (!pw_args_ok(dtype, M, N, K, pro_mode, scale, shift, gate, rows_per_frame)) return -1;
  const dfd::Pro pro{scale, shift, gate, rows_per_frame, K};
  hipStream_t s = (hipStream_t)stream;
  if (dtype == DFD_DTYPE_BF16)
    return dfd::launch_pw_gemm<dfd::bf16>(s, (const dfd::bf16*)A, (const dfd::bf16*)W, (dfd::bf16*)C,
                                          (const dfd::bf16*)R, M, N, K, pro_mode, pro, stats, stat_rows);
  if (dtype == DFD_DTYPE_F16)
    return dfd::launch_pw_gemm<dfd::f16>(s, (const dfd::f16*)A, (const dfd::f16*)W, (dfd::f16*)C, (const dfd::f16*)R,
                                         M, N, K, pro_mode, pro, stats, stat_rows);
  return dfd::launch_pw_gemm<float>(s, (const float*)A, (const float*)W, (float*)C, (const float*)R, M, N, K, pro_mode,
                                    pro, stats, stat_rows);
  DFD_GUARD_END
}

int dfd_attention(void* stream, int backward, int images, int heads, int nt, float scale, const void* qkv, int64_t ldq,
                  int koff, int voff, void* O, int64_t ldo, float* lse, const void* dO, int64_t lddo, void* dqkv,
                  int64_t lddq) {
  DFD_GUARD_BEGIN
  if (!qkv || !O || !lse || images < 1 || heads < 1 || !dfd::attn_supported(nt, 64) || (backward && (!dO || !dqkv))) {
    dfd::set_error("attention: bad arguments", __FILE__, __LINE__);
    return -1;
  }
  dfd::AttnArgs a{};
  a.images = images; a.heads = heads; a.nt = nt; a.scale = scale;
  a.qkv = (const dfd::bf16*)qkv; a.ldq = ldq; a.koff = koff; a.voff = voff;
  a.O = (dfd::bf16*)O; a.ldo = ldo; a.lse = lse;
  a.dO = (const dfd::bf16*)dO; a.lddo = lddo; a.dqkv = (dfd::bf16*)dqkv; a.lddq = lddq;
  return backward ? dfd::launch_attn_bwd((hipStream_t)stream, a) : dfd::launch_attn_fwd((hipStream_t)stream, a);
  DFD_GUARD_END
}

int64_t dfd_blaslt_calls(void) { return dfd::blaslt_calls(); }

int64_t dfd_vgemm_tn_slab_floats(int64_t M, int N, int K) {
  return (int64_t)dfd::vgemm_tn_splits(M, N, K, INT64_MAX) * ((int64_t)N * K + N);  // + the column sums
}

int dfd_vgemm(void* stream, int op, const void* A, const void* B, void* C, const void* R, const float* bias,
              const void* Z, void* G, int64_t M, int N, int K, int epi, float* slab, int64_t slab_floats) {
  DFD_GUARD_BEGIN
  const dfd::Tuning tn = seam_snapshot();  // a kernel test seam: the dfd_set_tuning overrides apply (vg_xp)
  const dfd::TuningScope ts(&tn);
  hipStream_t s = (hipStream_t)stream;
  if (!A || !B || !C) { dfd::set_error("vgemm: null argument", __FILE__, __LINE__); return -1; }
  if (op == 0 || op == 2 || op == 4 || op == 5 || op == 7) {  // NT: own kernel (0; 4 / 5 / 7: 256- / 128- / 64-wide tiles) or hipBLASLt (2)
    if (((epi & dfd::VG_BIAS) && !bias) || ((epi & dfd::VG_RESID) && !R) || ((epi & dfd::VG_DGELU) && !Z) ||
        ((epi & dfd::VG_GELU2) && !G)) {
      dfd::set_error("vgemm: epilogue operand missing", __FILE__, __LINE__);
      return -1;
    }
    if (op == 2) {
      if (epi & ~(dfd::VG_BIAS | dfd::VG_RESID)) { dfd::set_error("vgemm: library path takes bias/resid", __FILE__, __LINE__); return -1; }
      return dfd::blaslt_linear(s, (const dfd::bf16*)A, (const dfd::bf16*)B, (dfd::bf16*)C, (const dfd::bf16*)R,
                                bias, M, N, K);
    }
    dfd::VgemmArgs a{};
    a.A = (const dfd::bf16*)A; a.B = (const dfd::bf16*)B; a.C = (dfd::bf16*)C; a.R = (const dfd::bf16*)R;
    a.bias = bias; a.Z = (const dfd::bf16*)Z; a.G = (dfd::bf16*)G;
    a.lda = K; a.ldb = K; a.ldc = N; a.M = (int)M; a.N = N; a.K = K;
    a.bn = op == 4 ? 256 : op == 5 ? 128 : op == 7 ? 64 : 0;
    return dfd::launch_vgemm_nt(s, a, epi);
  }
  if (op == 1 || op == 3 || op == 6) {  // TN: C (fp32 [N][K]) = A^T . B with A [M][N], B [M][K]
    if (!slab) { dfd::set_error("vgemm: slab missing", __FILE__, __LINE__); return -1; }
    if (op == 6) {  // the cooperative split reduction (the ViT backward's form): counters from the slab's tail
      const int nb = dfd::vgemm_tn_bar_count(N, K);
      const int64_t cap = slab_floats - (nb + 64);
      if (nb <= 0 || cap <= 0) { dfd::set_error("vgemm: slab too small", __FILE__, __LINE__); return -1; }
      unsigned* bar = reinterpret_cast<unsigned*>(slab + cap);
      DFD_HIP_CHECK(hipMemsetAsync(bar, 0, (size_t)nb * sizeof(unsigned), s));
      return dfd::launch_vgemm_tn(s, (const dfd::bf16*)A, N, (const dfd::bf16*)B, K, M, N, K, slab, cap, (float*)C,
                                  false, (float*)G, bar);
    }
    if (op == 3)
      return dfd::blaslt_wgrad_split(s, (const dfd::bf16*)A, (const dfd::bf16*)B, (float*)C, M, N, K, 4, slab,
                                     slab_floats);
    return dfd::launch_vgemm_tn(s, (const dfd::bf16*)A, N, (const dfd::bf16*)B, K, M, N, K, slab, slab_floats,
                                (float*)C, false, (float*)G);
  }
  dfd::set_error("vgemm: op must be 0..6", __FILE__, __LINE__);
  return -1;
  DFD_GUARD_END
}

int dfd_sgemm(void* stream, int ta, int tb, const float* A, int lda, const float* B, int ldb, float* C, int ldc, int M,
              int N, int K, float beta, const float* bias) {
  DFD_GUARD_BEGIN
  if (!A || !B || !C || M < 0 || N < 0 || K < 0) { dfd::set_error("sgemm: bad arguments", __FILE__, __LINE__); return -1; }
  return dfd::launch_sgemm((hipStream_t)stream, ta != 0, tb != 0, A, lda, B, ldb, C, ldc, M, N, K, beta, bias);
  DFD_GUARD_END
}

int dfd_pw_conv_wgrad(void* stream, int dtype, const void* dY, const void* X, int64_t M, int N, int K, int pro_mode,
                      const float* scale, const float* shift, const float* gate, int rows_per_frame, float* slab,
                      int64_t slab_floats, float* dW, int accumulate) {
  DFD_GUARD_BEGIN
  const dfd::Tuning tn = seam_snapshot();
  const dfd::TuningScope ts(&tn);
  if (!pw_args_ok(dtype, M, N, K, pro_mode, scale, shift, gate, rows_per_frame)) return -1;
  if (!slab || slab_floats < (int64_t)N * K) { dfd::set_error("pw wgrad: slab smaller than N*K", __FILE__, __LINE__); return -1; }
  const dfd::Pro pro{scale, shift, gate, rows_per_frame, K};
  hipStream_t s = (hipStream_t)stream;
  if (dtype == DFD_DTYPE_BF16)
    return dfd::launch_pw_wgrad<dfd::bf16>(s, (const dfd::bf16*)dY, (const dfd::bf16*)X, M, N, K, pro_mode, pro, slab,
                                           slab_floats, dW, accumulate != 0);
  if (dtype == DFD_DTYPE_F16)
    return dfd::launch_pw_wgrad<dfd::f16>(s, (const dfd::f16*)dY, (const dfd::f16*)X, M, N, K, pro_mode, pro, slab,
                                          slab_floats, dW, accumulate != 0);
  return dfd::launch_pw_wgrad<float>(s, (const float*)dY, (const float*)X, M, N, K, pro_mode, pro, slab, slab_floats,
                                     dW, accumulate != 0);
  DFD_GUARD_END
}

}  // extern "C"

// ---------------------------------------------------------------- LogicRNNLSTM
static bool rnn_dims_ok(int B, int T, int IN, int H, int L) {
  if (B <= 0 || T <= 0 || IN <= 0 || H <= 0 || L < 1 || L > 8) {
    dfd::set_error("rnn: bad dimensions", __FILE__, __LINE__);
    return false;
  }
  return true;
}

int64_t dfd_rnn_work_floats(int B, int T, int IN, int H, int L) {
  DFD_GUARD_BEGIN
  if (!rnn_dims_ok(B, T, IN, H, L)) return -1;
  return dfd::rnn_work_floats(dfd::RnnDims{B, T, IN, H, L});
  DFD_GUARD_END
}

int64_t dfd_rnn_scratch_floats(int B, int T, int IN, int H, int L) {
  DFD_GUARD_BEGIN
  if (!rnn_dims_ok(B, T, IN, H, L)) return -1;
  return dfd::rnn_scratch_floats(dfd::RnnDims{B, T, IN, H, L});
  DFD_GUARD_END
}

int dfd_rnn_forward(void* stream, int B, int T, int IN, int H, int L, const float* x, const int64_t* order,
                    const int64_t* lengths, float* const* params, float* work, float* y, uint64_t seed, float p) {
  DFD_GUARD_BEGIN
  if (!rnn_dims_ok(B, T, IN, H, L)) return -1;
  if (!x || !params || !work || !y) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  dfd::RnnParams P{};
  if (dfd::rnn_params_from_table(params, L, P)) return -1;
  return dfd::rnn_forward((hipStream_t)stream, dfd::RnnDims{B, T, IN, H, L}, P, x, order, lengths, work, y, seed, p);
  DFD_GUARD_END
}

int dfd_rnn_backward(void* stream, int B, int T, int IN, int H, int L, const float* x, const int64_t* order,
                     const int64_t* lengths, float* const* params, float* work, float* scratch, const float* dy,
                     float* const* grads, uint64_t seed, float p) {
  DFD_GUARD_BEGIN
  if (!rnn_dims_ok(B, T, IN, H, L)) return -1;
  if (!x || !params || !work || !scratch || !dy || !grads) { dfd::set_error("null argument", __FILE__, __LINE__); return -1; }
  dfd::RnnParams P{}, G{};
  if (dfd::rnn_params_from_table(params, L, P) || dfd::rnn_params_from_table(grads, L, G)) return -1;
  return dfd::rnn_backward((hipStream_t)stream, dfd::RnnDims{B, T, IN, H, L}, P, x, order, lengths, work, scratch, dy,
                           G, seed, p);
  DFD_GUARD_END
}
