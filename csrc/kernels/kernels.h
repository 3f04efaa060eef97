// Launchers for the gfx950 kernels (reduce.hip, counts.hip, optim.hip,
// pack_bf16.hip, colsum.hip, xent.hip).
#pragma once

#include <hip/hip_runtime.h>

#include "../engine/device.h"

namespace akka {

enum class ReduceImpl : int32_t {
  Auto = 0,     // pick per call from the working set (profiles/README.md)
  Vec = 1,      // 16-B global loads straight to VGPRs; load/store policy picked per call
  Lds = 2,      // global_load_lds (LDS-DMA) double-buffered staging, then ds_read + sum
  Scalar = 3,   // unaligned fallback
  VecNts = 4,   // vec, plain loads + nontemporal stores (inputs stay in the Infinity Cache)
  VecNtl = 5,   // vec, nontemporal loads + plain stores
  VecBoth = 6,  // vec, nontemporal loads and stores, unroll 2 (large streams)
};
ReduceImpl reduce_impl_from_name(const char* name);

// dst = sum(srcs) over n elements (fp32 accumulate).
void launch_reduce(hipStream_t s, const ReduceSpec& spec, DType dt, ReduceImpl impl);
// A round's contributor counts[N][kmax] (per block, per chunk) and their layout: what every count pass walks.
struct CountsTable {
  const int32_t* counts;
  int64_t S, step;
  int32_t N;
  int64_t C;
  int32_t kmax;
  int64_t regions() const { return int64_t(N) * kmax; }
  void check(const char* who) const {
    AKKA_CHECK(regions() > 0 && step >= 0 && C > 0, std::string(who) + ": bad geometry");
  }
};
// counts -> out[S] (per element), RB:41-47.
void launch_count_expand(hipStream_t s, int32_t* out, const CountsTable& t);
// dst = src / per-chunk count (0 where the count is 0), one pass; with
// `axpy`: dst += alpha * that mean (fused SGD update).  dt is the
// destination's dtype, src_dt the source's: the same, or bf16 into fp32 (the
// sum of a compressed wire read straight into fp32 gradients / parameters).
void launch_count_mean(hipStream_t s, void* dst, const void* src, const CountsTable& t, DType dt, DType src_dt,
                       bool axpy = false, float alpha = 0.f, void* shadow = nullptr);
// The fused optimizer step over a round's output (optim.hip).  Per element
// g = src / per-chunk count, times min(1, max_norm / (sqrt(*sq) + 1e-6)) when
// `sq` is given, then torch.optim.SGD's update (momentum, dampening 0) or
// torch.optim.AdamW's on fp32 p, m (and v); bf16(p_new) into `shadow` if
// given.  A chunk whose count is 0 is missing: p, m, v, shadow stay as they
// are.  `t`: the step, one int32 on the device (AdamW's bias corrections).
// src_dt: F32 or BF16.  nt: nontemporal instead of plain accesses (slower
// where measured; for the comparison in bench/fused_opt.py).
// state_dt: the element type of m and v, F32 or BF16.  BF16 moments are widened
// on load, updated in fp32 and stored with stochastic rounding, the bits drawn
// from (element index, *t, seed) -- the definition is in optim.hip; p and the
// shadow come from the unrounded moments.  `t` is then needed for SGD too, and
// nt is refused.  seed is not used with F32 state.
// param_dt: the element type of p, F32 or BF16.  BF16 parameters need BF16
// state and take neither a shadow nor nt (refused).  They are widened on load,
// everything is computed as for an fp32 p of that value, and the store of p is
// rounded stochastically with a second hash of (element index, *t, seed).
//
// LAMB: AdamW's m and v, u = (m / bc1) / (sqrt(v / bc2) + eps) + wd * p and
// p -= lr * r * u with one trust ratio r per layer.  It runs with groups only,
// one segment per layer, and takes r from groups->trust, which
// launch_lamb_norms and launch_lamb_trust (below) fill before it.
enum class OptimKind : int32_t { SGD = 0, AdamW = 1, LAMB = 2 };
struct OptimSpec {
  OptimKind kind = OptimKind::SGD;
  double lr = 0, weight_decay = 0;
  double momentum = 0;  // SGD
  bool nesterov = false;
  double beta1 = 0.9, beta2 = 0.999, eps = 1e-8;  // AdamW, LAMB
  double max_norm = 0;                            // used with sq
};
// With `groups` the flat buffer is cut into `nseg` segments with one group's
// learning rate and weight decay each: seg_end (device, int64) holds their
// ascending exclusive ends, the last one S, seg_group (device, int32) each
// segment's group in [0, ngroups); host_seg_end / host_seg_group are the host
// copies the launcher checks.  rows (device, float[ngroups][4], 16-B aligned) =
// {float(-lr_g), float(wd_g), float(lr_g), float(1 - lr_g * wd_g)} per group,
// read when the kernel RUNS: rewriting them between the replays of a captured
// step changes its schedule.  o.lr and o.weight_decay are then not used, and nt
// is refused.  A group whose lr is 0 advances m and v and leaves p (times its
// decay of 1) in place.
struct OptimBuffers {
  void* p = nullptr;
  void *m = nullptr, *v = nullptr;
  DType state_dt = DType::F32;
  void* shadow = nullptr;
  const void* src = nullptr;
  DType src_dt = DType::F32;
  const int32_t* t = nullptr;
  const float* sq = nullptr;
  uint32_t seed = 0;
  // the norm pass's verdict (launch_count_sqnorm with a guard), or null: where guard[0] is 0 the pass returns
  // before its first load.  Needs sq and t; the norm pass has then advanced t, not the caller.
  const int32_t* guard = nullptr;
  // the element type of p, F32 or BF16.  BF16 parameters (with BF16 state only, no shadow, no nt) are widened on
  // load, updated in fp32 and stored with stochastic rounding from a second hash of (index, *t, seed): optim.hip
  DType param_dt = DType::F32;
};
struct OptimGroups {
  const int64_t* seg_end = nullptr;
  const int32_t* seg_group = nullptr;
  const float* rows = nullptr;
  int32_t nseg = 0, ngroups = 0;
  const int64_t* host_seg_end = nullptr;
  const int32_t* host_seg_group = nullptr;
  const float* trust = nullptr;  // LAMB: device, float[nseg], one trust ratio per segment
};
void launch_count_optim(hipStream_t s, const OptimBuffers& b, const CountsTable& ct, const OptimSpec& o,
                        const OptimGroups* groups = nullptr, bool nt = false);
// sq[0] = sum over the elements whose count is > 0 of (src / count)^2.  part:
// fp32 [count_sqnorm_partials()] workspace; ticket: one uint32 zeroed once
// (each launch leaves it zero again).  Deterministic for a given shape.
// guard (int32[4], zeroed once) and t (the step), both or neither: the pass
// judges the step by sq[0].  Finite: guard[0] = 1, guard[2] = 0, *t += 1.
// Otherwise: guard[0] = 0, guard[1] and guard[2] += 1, t as it is.  guard[3]
// is reserved.  sq[0] has the same bits with and without a guard.
void launch_count_sqnorm(hipStream_t s, float* sq, const void* src, DType src_dt, const CountsTable& ct, float* part,
                         uint32_t* ticket, int32_t* guard = nullptr, int32_t* t = nullptr);
int32_t count_sqnorm_partials();
// LAMB's per-layer norms, in two kernels; a layer is a segment of `groups`.
// launch_lamb_norms reads the sum, the counts, p, m, v, t, sq and the group
// rows (b, o, ct as for launch_count_optim; it writes none of them) and
// computes per element the new moments and u exactly as the update pass will.
// The flat buffer is cut into tiles of lamb_tile() elements; the sums of p^2
// and of u^2 over a (tile, layer) intersection, count-0 chunks left out, go to
// part[2 * (tile + layer)] and the float behind it.  part: 8-B aligned, `slots`
// pairs, at least tiles + layers of them; nothing in it needs a reset, ever.
// grid: workgroups (0: the launcher's choice); the partials do not depend on it.
// launch_lamb_trust (one workgroup per layer) sums a layer's partials in slot
// order and writes trust[layer] = ||p|| / ||u|| where both squared sums are
// positive and finite, else 1; 1 too where adapt[layer] (device, int32) is 0.
// With a guard whose verdict is "skipped" both kernels return at once.
int32_t lamb_tile();
void launch_lamb_norms(hipStream_t s, const OptimBuffers& b, const CountsTable& ct, const OptimSpec& o,
                       const OptimGroups& groups, float* part, int64_t slots, int32_t grid = 0);
void launch_lamb_trust(hipStream_t s, float* trust, const float* part, int64_t slots, const OptimGroups& groups,
                       int64_t S, const int32_t* adapt, const int32_t* guard = nullptr);
// q (bf16) = rne(g + r), r = (g + r) - float(q) in place; r may be null (a
// plain cast).  r becomes 0 where the sum or its rounding is not finite.
void launch_pack_bf16(hipStream_t s, void* q, const float* g, float* r, int64_t n);
// out[c] = sum_r in[r, c] (bf16 [M, ncol] row-major, fp32 out): the bias
// gradient.  part: fp32 [splits, ncol] workspace; tickets: uint32
// [ceil(ncol / 512)] zeroed once (each launch leaves them zero again).
// act / gout (both or neither, bf16 [M, ncol]): ReLU backward fused in --
// gout = in where act > 0 else 0, and out sums gout.
void launch_colsum_bf16(hipStream_t s, float* out, const void* in, int64_t M, int64_t ncol, float* part,
                        uint32_t* tickets, int32_t splits, bool lite = true, const void* act = nullptr,
                        void* gout = nullptr);
int32_t colsum_row_splits(int64_t M, int64_t ncol);
// Cross entropy over bf16 logits [B, C] with int64 labels (mean over the rows
// whose label is in [0, C)).  Forward: lse [B] fp32, rowloss [2B] fp32
// workspace, out [2] = {loss, valid rows}, ticket: one uint32 zeroed once.
// Backward: gx [B, C] bf16 = d(loss)/d(x) * go[0].
void launch_xent_fwd(hipStream_t s, const void* x, const int64_t* y, int64_t B, int64_t C, float* lse,
                     float* rowloss, float* out, uint32_t* ticket);
void launch_xent_bwd(hipStream_t s, const void* x, const int64_t* y, int64_t B, int64_t C, const float* lse,
                     const float* stat, const float* go, void* gx);
// counts[0..n) = 0 if *flag != 0 (read when the kernel runs): poisons the
// counts of a one-sided round whose waits failed.
void launch_poison_counts(hipStream_t s, const uint32_t* flag, int32_t* counts, int64_t n);
// counts[0..n) = (*flag != 0 ? 0 : value): fill + poison of an exact round in one launch.
void launch_fill_counts(hipStream_t s, const uint32_t* flag, int32_t* counts, int32_t value, int64_t n);
// Standalone kernels for tests/bench: out = a (+ b ...) via a pointer table on device.
ReduceImpl reduce_impl_from_env();
const char* reduce_impl_name(ReduceImpl i);

}  // namespace akka
