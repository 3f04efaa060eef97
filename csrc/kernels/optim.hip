// gfx950 kernels of the fused optimizer step over a round's output: momentum
// SGD, AdamW and LAMB straight from the reduced sum and its per-(block, chunk)
// contributor counts, with an optional global-norm clip.
//
// count_optim: one pass.  Per element g = sum / count(chunk), scaled by the
// clip coefficient, then torch's update (torch.optim.SGD with dampening 0,
// torch.optim.AdamW), operation by operation in the order and with the
// roundings of torch's own element-wise kernels (update_one below), so torch
// in fp32 is a comparator that differs in the last bits only.  p is fp32; m
// and v are fp32, or bf16 stored with stochastic rounding (below, in front of
// update_range); the sum is fp32 or bf16 (a compressed wire's sum, read wide
// into fp32); an optional bf16 shadow receives bf16(p_new) from the same pass.
// p may be bf16 too (a model trained in pure bf16; with bf16 moments only, no
// shadow: p is the weight the forward reads): widened on load, the same fp32
// arithmetic, the store rounded stochastically ("bf16 parameters" below).
//
// Count 0 means MISSING, not zero: a chunk no contributor reached leaves p, m,
// v and the shadow untouched -- the region is skipped before any load.  With
// plain SGD a missing gradient and a zero gradient give the same parameters;
// with momentum or Adam they do not (m would decay and still move p, v would
// decay), and a parameter must not drift on stale momentum because a
// threshold round dropped its chunk.  The bias corrections use the GLOBAL
// step t (read from device memory: a captured step advances it on every
// replay), also for a chunk that missed earlier steps: its m and v are then
// older than t says, which only shortens its next steps.
//
// Region walk as count_mean (counts.hip): one workgroup per (block, chunk)
// region at a time, the count a wave-uniform scalar, gridDim.y workgroups
// sharing a region while there are few.  A unit is 8 elements: one 16-B
// vector of a bf16 sum or two of an fp32 one, two each of fp32 p, m and v, one
// each of bf16 ones, one of the shadow -- every stream moves 16 B per access.  Elements of a region
// outside its 8-aligned body go through the scalar path.  Two units per
// thread, every load of both in flight before the first store.
//
// Cache policy.  Bytes per element (fp32 sum; 2 less from a bf16 one):
// SGD 20 (+2 shadow), AdamW 28 (+2 shadow).  At the config-5 bucket (41.75 M
// elements, 0.75-1.25 GB per pass, far past the 256 MiB Infinity Cache) plain
// loads and stores measured 4.7-5.3 TB/s of these bytes and nontemporal ones
// 2.7-4.2 TB/s in every variant (AdamW + shadow from an fp32 sum: 237 us
// against 309 us), so unlike pack_bf16 this pass uses plain accesses at every
// size; `nt` is kept so that bench/fused_opt.py can repeat the comparison
// (table in profiles/r08/fused_opt/README.md).  bf16 moments take 4 B per
// element off SGD and 8 B off AdamW, and the time follows the bytes
// (profiles/r10/bf16_state/README.md).  bf16 parameters take 4 B more off
// either and the shadow's 2 B with them; from a bf16 sum, per element:
//                                      sum  p  m  v  shadow  total
//   AdamW, bf16 moments, fp32 p         2   8  4  4    2      20
//   AdamW, bf16 moments, bf16 p         2   4  4  4    -      14
//   SGD,   bf16 moments, fp32 p         2   8  4  -    2      16
//   SGD,   bf16 moments, bf16 p         2   4  4  -    -      10
// Plain accesses only, as for bf16 moments: there is no nontemporal variant
// (profiles/r13/bf16_params/README.md has the times).
//
// With a group table the same kernel takes each group's weight decay and
// learning rate from a small device table when it runs (below, at the kernel);
// numbers in profiles/r09/param_groups/README.md.
//
// count_sqnorm: sq[0] = sum over count > 0 of (sum / count)^2, the squared
// global norm of the mean gradient the clip needs.  fp32 partials per thread,
// a fixed wave + workgroup tree, one partial per workgroup written through
// (sc0 sc1) into a workspace; the last workgroup to draw the ticket sums the
// partials in index order and re-arms the ticket (the colsum / xent hand-off:
// no float atomics, no waits).  Same bits for the same shape on every call,
// and nothing to reset between the replays of a graph.
//
// Skipping a non-finite step.  With a guard record (int32[4], zeroed once:
// {last pass applied, steps skipped in total, skipped in a row, 0}) the norm
// pass also gives the verdict: the thread that stores sq[0] tests the sum's
// exponent bits and writes the record with plain stores.  Finite: applied,
// and it advances the step t -- with a guard the pass owns the step, the caller
// does not advance it.  Not finite (a NaN or an inf in a chunk with a
// contributor, or a squared norm that overflows fp32): skipped, counted, t
// stays.  count_optim with the guard returns before its first load in every
// workgroup of a skipped step, so p, m, v, the shadow and t keep their bits,
// and the bias corrections and the rounding key see a run with a skipped step
// exactly as a run in which that round never happened.  Without a guard both
// kernels do what they did before it existed.
//
// LAMB.  AdamW's m and v, then per layer L (a segment of the group table, one
// per parameter)
//   u = (m / bc1) / (sqrt(v / bc2) + eps) + wd * p,   r_L = ||p||_L / ||u||_L,
//   p = p - lr * r_L * u
// (the fp32 operation order: at update_one).  r_L is 1 unless both norms are
// positive and finite, and 1 for a layer that opted out.  Both norms run over
// the layer's elements whose count is > 0, p before the step: a missing chunk
// enters neither, and a layer without a contributor keeps r = 1 and does not
// move.  Three launches: lamb_norms, lamb_trust, count_optim<LAMB>.
// lamb_norms (at the kernel) recomputes m_new, v_new and u per element in
// registers with the update's own device function -- the u that is normed and
// the u that is applied are the same bits, with bf16 moments too -- and leaves
// one pair of partial sums per (tile, layer) intersection, each in a slot of
// its own; it writes nothing else.  It reads 16 B per element (fp32 sum and
// state), the update 30: 46 against AdamW's 30, and the step measured 1.44-1.45x
// an AdamW step at the config-5 bucket (profiles/r12/fused_lamb/README.md).
// lamb_trust turns a layer's partials into r_L with one workgroup per layer and
// a fixed-order sum.  A second kernel and not count_sqnorm's ticket: the kernel
// boundary is the hand-off, so there is no ticket to re-arm and no
// written-through partial, and the sum's order is tied to the slots, not to
// which workgroup arrived last -- the result cannot depend on lamb_norms' grid.
// The ticket would save one launch of ~10 us in a 400 us step and would need one
// ticket per layer.  No float atomics, no host sync, nothing to reset between
// launches or replays; same bits for the same inputs on every call.  With the
// guard, count_sqnorm runs first and owns t as for the other kinds; after a
// skipped step lamb_norms and lamb_trust return at once too, so the trust table
// keeps the last applied step's ratios.
#include <hip/hip_runtime.h>

#include "elem.h"
#include "kernels.h"
#include "launch_util.h"
#include "xgmi_device.h"

namespace akka {

namespace {

// The kind of update as a template argument (OptimKind's values).
enum : int { kSGD = 0, kAdam = 1, kLamb = 2 };

// Host-rounded scalars of one step (each the fp32 torch's kernels receive).
struct OptimK {
  float neg_lr, wd, mu;  // SGD
  int32_t nesterov;
  float lr, decay, b1, w1, b2, w2, eps;  // AdamW: decay = 1 - lr * wd, w_k = 1 - b_k
  float max_norm;
};

// Wave-uniform values read from device memory when the kernel runs.
struct Coef {
  float clip;    // gradient scale
  float d1, d2;  // AdamW: p += m / (sqrt(v) / d1 + d2); LAMB: u = (m * d1) / (sqrt(v) / d2 + eps) + wd * p
  bool move;     // with a group table: false for a group whose learning rate is 0
  float step;    // LAMB: -(lr * r), the layer's trust ratio r folded into the group's learning rate
};

// The part of them that does not depend on the learning rate: once per kernel.
struct StepCoef {
  float clip;
  float inv_bc1, sbc2;  // AdamW: 1 / (1 - b1^t), sqrt(1 - b2^t)
};

template <int KIND>
__device__ __forceinline__ StepCoef step_coefficients(const OptimK& k, const int32_t* t, const float* sq) {
#pragma clang fp contract(off)
  constexpr bool ADAM = KIND != kSGD;  // AdamW and LAMB: the moments and their bias corrections
  StepCoef c{1.f, 0.f, 0.f};
  // clip_grad_norm_: min(1, max_norm / (norm + 1e-6)), the quotient as reciprocal * max_norm
  if (sq) c.clip = fminf(1.f, (1.f / (sqrtf(*sq) + 1e-6f)) * k.max_norm);
  if constexpr (ADAM) {
    // AdamW(capturable=True): bc_k = 1 - b_k^t in fp32
    const float tf = float(*t);
    c.inv_bc1 = 1.f / (1.f - powf(k.b1, tf));
    c.sbc2 = sqrtf(1.f - powf(k.b2, tf));
  }
  return c;
}

// The part that does: once per kernel, or per group sub-range with a group table.
// r: the layer's trust ratio (LAMB only).
template <int KIND>
__device__ __forceinline__ Coef lr_coefficients(const StepCoef& sc, float lr, float eps, float r = 1.f) {
#pragma clang fp contract(off)
  Coef c{sc.clip, 0.f, 0.f, lr != 0.f};
  if constexpr (KIND == kLamb) {
    c.d1 = sc.inv_bc1;
    c.d2 = sc.sbc2;
    c.step = -(lr * r);
  }
  if constexpr (KIND == kAdam) {
    // the step size lr / bc1 and sqrt(bc2) folded into the denominator, eps scaled to match:
    // p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
    const float nss = -(sc.inv_bc1 * lr);
    c.d1 = sc.sbc2 * nss;
    c.d2 = (1.f / nss) * eps;
  }
  return c;
}

// One element.  No contraction but the fused multiply-adds spelled out: they
// are the ones torch's add(alpha) / lerp / addcmul kernels make.  GROUPS: a
// group whose learning rate is 0 (a schedule's first step; c.move is false,
// wave-uniform) advances the state, gives p its decay (a factor of 1) and no
// step -- the step's formula is 0 / -0 there while v is 0.
//
// LAMB (k.wd: the group's decay; c: lr_coefficients<kLamb>), in this order in fp32:
//   g  = g * clip
//   m, v as AdamW's, by the same function (adam_moments)
//   u  = (m * inv_bc1) / (sqrt(v) / sbc2 + eps)        inv_bc1 = 1 / (1 - b1^t), sbc2 = sqrt(1 - b2^t)
//   u  = fma(wd, p, u)                                  lamb_u: the norm pass and the update share it
//   p  = fma(-(lr * r), u, p)                           r: the layer's trust ratio; not where lr == 0
__device__ __forceinline__ void adam_moments(float g, float& m, float& v, const OptimK& k) {
#pragma clang fp contract(off)
  const float d = g - m;  // m = b1 * m + (1 - b1) * g as lerp_ spells it
  m = k.w1 < 0.5f ? __builtin_fmaf(k.w1, d, m) : __builtin_fmaf(-d, 1.f - k.w1, g);
  v = __builtin_fmaf(k.w2, g * g, v * k.b2);
}

// g: the mean gradient before the clip.  m and v become the new moments; returns u.
__device__ __forceinline__ float lamb_u(float g, float p, float& m, float& v, const OptimK& k, const Coef& c) {
#pragma clang fp contract(off)
  g = g * c.clip;
  adam_moments(g, m, v, k);
  const float u = (m * c.d1) / (sqrtf(v) / c.d2 + k.eps);
  return __builtin_fmaf(k.wd, p, u);
}

template <int KIND, bool GROUPS = false>
__device__ __forceinline__ void update_one(float g, float& p, float& m, float& v, const OptimK& k, const Coef& c) {
#pragma clang fp contract(off)
  if constexpr (KIND == kLamb) {
    const float u = lamb_u(g, p, m, v, k, c);
    if (c.move) p = __builtin_fmaf(c.step, u, p);
    return;
  }
  g = g * c.clip;
  if constexpr (KIND == kAdam) {
    p = p * k.decay;
    adam_moments(g, m, v, k);
    if (!GROUPS || c.move) p = p + m / (sqrtf(v) / c.d1 + c.d2);
  } else {
    g = __builtin_fmaf(k.wd, p, g);
    m = m * k.mu + g;
    if (!GROUPS || c.move) {
      if (k.nesterov) g = __builtin_fmaf(k.mu, m, g);
      else g = m;
      p = __builtin_fmaf(k.neg_lr, g, p);
    }
  }
}

// bf16 moments (TM = bf16_t): m and v are stored as bf16 and rounded
// STOCHASTICALLY.  Round-to-nearest is not an option: v = b2 * v + (1 - b2) *
// g^2 moves by 2^-10 of itself per step at b2 = 0.999 and a bf16 ulp is 2^-8 of
// the value, so a nearest-rounded v stops where the increment falls under half
// an ulp (g = 1: at 0.25 instead of 0.632 after 1000 steps).  With the rounding
// below the expectation of the stored value is the fp32 value.
//
// Definition (x fp32, r 16 bits; the tests carry their own copy of it):
//   sr(x, r) = uint16((bits(x) + r) >> 16)   for finite x,
//              Elt<bf16_t>::from_f(x)        otherwise          (sr_bf16, elem.h)
//   mix(x)   : x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b;
//              x ^= x >> 16                   on uint32          (mix32, elem.h)
//   key      = mix(seed ^ mix(uint32(*t)))
//   h(i)     = mix(uint32(i) ^ (uint32(i >> 32) * 0x9e3779b9) ^ key)
//              for the element's flat index i (int64) in the bucket
//   m takes r = h & 0xffff, v takes r = h >> 16.
// The bits depend on (index, device step, seed) and on nothing else: every
// rank of a data-parallel job rounds alike (with the same seed), a captured
// step draws new bits on each replay (*t is read when the kernel runs), and
// neither the grid nor the chunk geometry matters.  The key is wave-uniform,
// computed once per kernel.
//
// The pass widens m and v exactly on load, runs update_one on the fp32 values
// and computes p and the shadow from the UNROUNDED new moments: only the stores
// of m and v go through sr, so p is bitwise what the fp32-state pass gives from
// the widened state.  A unit is still 8 elements, m and v one 16-B vector each.
// Nontemporal accesses are not offered with bf16 moments (the launcher refuses).
//
// bf16 parameters (TP = bf16_t; with bf16 moments only, no shadow, no
// nontemporal variant -- the launcher refuses the rest and no other
// instantiation exists).  p is one 16-B vector per unit, loaded with the other
// streams, widened exactly (unit_elem), and update_one, lamb_u and the
// coefficients run on the widened value as they are: m and v get the bits the
// fp32-p pass gives from that value.  Only the store of p is rounded, and
// stochastically for the reason given for v: lr * u = 1e-4 at p = 1 is 1/39 of
// a bf16 ulp, and a nearest-rounded parameter never moves.  Definition, with
// h(i), mix and sr from above:
//   h2(i) = mix(h(i) ^ 0x85ebca6b)
//   p takes r = h2(i) & 0xffff;   stored p = sr(p_new, r)
// A second hash and not a third slice of h: h has 32 bits and m and v use them
// all.  h2 depends on (index, device step, seed) alone, like h.  An element
// whose fp32 p_new equals its widened old p (a zero update; a group at lr == 0,
// where AdamW's decay factor is exactly 1) keeps its bits: the low 16 bits of
// p_new are zero and r < 2^16 carries nothing.  Count-0 regions and a skipped
// step return before any load, as ever.  LAMB's norm pass reads the same
// widened p, before the step.
__device__ __forceinline__ uint32_t sr_key(uint32_t seed, const int32_t* t) {
  return mix32(seed ^ mix32(uint32_t(*t)));
}

// The index's part of h: everything but the last mix, for an index whose low 32 bits are lo.
__device__ __forceinline__ uint32_t sr_hi(int64_t i, uint32_t key) {
  return (uint32_t(uint64_t(i) >> 32) * 0x9e3779b9u) ^ key;
}

// h2 from the element's h: the bits of a bf16 parameter's store.
__device__ __forceinline__ uint32_t sr_h2(uint32_t h) { return mix32(h ^ 0x85ebca6bu); }

// The elements [s, e) of one count region (fv: its count) with one set of
// scalars: scalar head and tail outside the 8-aligned body, units in between,
// split over the gridDim.y workgroups that share the region.  TM: the element
// type of m and v; TP: that of p; key: the rounding key (bf16 moments only).
template <typename TS, typename TM, typename TP, int KIND, bool SHADOW, bool NT, bool GROUPS = false>
__device__ __forceinline__ void update_range(TP* __restrict__ p, TM* __restrict__ m, TM* __restrict__ v,
                                             bf16_t* __restrict__ shadow, const TS* __restrict__ src, int64_t s,
                                             int64_t e, float fv, const OptimK& k, const Coef& c, uint32_t key) {
  constexpr bool ADAM = KIND != kSGD;          // a second moment
  constexpr bool SR = Elt<TM>::kPerVec == 8;  // bf16 moments, stored with stochastic rounding
  constexpr bool PB = Elt<TP>::kPerVec == 8;  // bf16 parameters: widened on load, the store rounded with h2
  static_assert(!(SR && NT), "bf16 moments have no nontemporal variant");
  static_assert(!PB || (SR && !SHADOW), "bf16 parameters: bf16 moments, no shadow");
  constexpr int E = 8;                        // elements per unit
  constexpr int ES = Elt<TS>::kPerVec;        // elements per source vector
  constexpr int NS = E / ES;                  // source vectors per unit
  constexpr int NF = E / Elt<float>::kPerVec; // fp32 vectors per unit and stream
  constexpr int NM = E / Elt<TM>::kPerVec;    // vectors of m (and of v) per unit
  constexpr int NP = E / Elt<TP>::kPerVec;    // vectors of p per unit
  int64_t a = (s + E - 1) & ~int64_t(E - 1);  // first element 16-B aligned in every stream
  if (a > e) a = e;
  const int64_t nv = (e - a) / E;
  auto one = [&](int64_t i) {
    float pi = Elt<TP>::to_f(p[i]), mi = Elt<TM>::to_f(m[i]), vi = ADAM ? Elt<TM>::to_f(v[i]) : 0.f;
    update_one<KIND, GROUPS>(Elt<TS>::to_f(src[i]) / fv, pi, mi, vi, k, c);
    if constexpr (SR) {
      const uint32_t h = mix32(uint32_t(i) ^ sr_hi(i, key));
      if constexpr (PB) p[i] = sr_bf16(pi, sr_h2(h) & 0xffffu);
      else p[i] = pi;
      m[i] = sr_bf16(mi, h & 0xffffu);
      if constexpr (ADAM) v[i] = sr_bf16(vi, h >> 16);
    } else {
      p[i] = pi;
      m[i] = mi;
      if constexpr (ADAM) v[i] = vi;
    }
    if constexpr (SHADOW) shadow[i] = Elt<bf16_t>::from_f(pi);
  };
  if (blockIdx.y == 0) {
    for (int64_t i = s + threadIdx.x; i < a; i += kBlock) one(i);
    for (int64_t i = a + nv * E + threadIdx.x; i < e; i += kBlock) one(i);
  }
  const v4u* s4 = reinterpret_cast<const v4u*>(src + a);
  v4u* p4 = reinterpret_cast<v4u*>(p + a);
  v4u* m4 = reinterpret_cast<v4u*>(m + a);
  v4u* v4 = reinterpret_cast<v4u*>(v + a);
  v4u* h4 = reinterpret_cast<v4u*>(shadow + a);
  auto ld = [](const v4u* q) { return NT ? __builtin_nontemporal_load(q) : *q; };
  auto st = [](const v4u& x, v4u* q) {
    if constexpr (NT) __builtin_nontemporal_store(x, q);
    else *q = x;
  };
  struct Unit {
    v4u s[NS], p[NP], m[NM], v[NM];
  };
  auto load = [&](int64_t at) {
    Unit u;
#pragma unroll
    for (int q = 0; q < NS; ++q) u.s[q] = ld(s4 + at * NS + q);
#pragma unroll
    for (int q = 0; q < NP; ++q) u.p[q] = ld(p4 + at * NP + q);
#pragma unroll
    for (int q = 0; q < NM; ++q) u.m[q] = ld(m4 + at * NM + q);
    if constexpr (ADAM) {
#pragma unroll
      for (int q = 0; q < NM; ++q) u.v[q] = ld(v4 + at * NM + q);
    }
    return u;
  };
  auto update = [&](Unit& u, int64_t at) {
    float g[E], pn[E];
#pragma unroll
    for (int q = 0; q < E; ++q) g[q] = 0.f;
#pragma unroll
    for (int q = 0; q < NS; ++q) Elt<TS>::add(reinterpret_cast<float(&)[ES]>(g[q * ES]), u.s[q]);
    if constexpr (SR) {
      // the unit's first element is a multiple of 8: its elements differ in the low three bits alone
      const int64_t i0 = a + at * E;
      const uint32_t lo = uint32_t(i0), hi = sr_hi(i0, key);
      uint32_t mo[E], vo[E];
      [[maybe_unused]] uint32_t po[PB ? E : 1];  // bf16 p: the rounded halves
#pragma unroll
      for (int q = 0; q < E; ++q) {
        float pi, mi = unit_elem<TM>(u.m, q);
        if constexpr (PB) pi = unit_elem<TP>(u.p, q);
        else pi = __uint_as_float(u.p[q >> 2][q & 3]);
        float vi = ADAM ? unit_elem<TM>(u.v, q) : 0.f;
        update_one<KIND, GROUPS>(g[q] / fv, pi, mi, vi, k, c);
        pn[q] = pi;
        if constexpr (!PB) u.p[q >> 2][q & 3] = __float_as_uint(pi);
        const uint32_t h = mix32((lo | uint32_t(q)) ^ hi);
        if constexpr (PB) po[q] = sr_bf16(pi, sr_h2(h) & 0xffffu);
        mo[q] = sr_bf16(mi, h & 0xffffu);
        if constexpr (ADAM) vo[q] = sr_bf16(vi, h >> 16);
      }
      if constexpr (PB) {
        st(v4u{po[0] | (po[1] << 16), po[2] | (po[3] << 16), po[4] | (po[5] << 16), po[6] | (po[7] << 16)}, p4 + at);
      } else {
#pragma unroll
        for (int q = 0; q < NF; ++q) st(u.p[q], p4 + at * NF + q);
      }
      st(v4u{mo[0] | (mo[1] << 16), mo[2] | (mo[3] << 16), mo[4] | (mo[5] << 16), mo[6] | (mo[7] << 16)}, m4 + at);
      if constexpr (ADAM)
        st(v4u{vo[0] | (vo[1] << 16), vo[2] | (vo[3] << 16), vo[4] | (vo[5] << 16), vo[6] | (vo[7] << 16)}, v4 + at);
    } else {
#pragma unroll
      for (int q = 0; q < E; ++q) {
        float pi = __uint_as_float(u.p[q >> 2][q & 3]), mi = __uint_as_float(u.m[q >> 2][q & 3]);
        float vi = ADAM ? __uint_as_float(u.v[q >> 2][q & 3]) : 0.f;
        update_one<KIND, GROUPS>(g[q] / fv, pi, mi, vi, k, c);
        pn[q] = pi;
        u.p[q >> 2][q & 3] = __float_as_uint(pi);
        u.m[q >> 2][q & 3] = __float_as_uint(mi);
        if constexpr (ADAM) u.v[q >> 2][q & 3] = __float_as_uint(vi);
      }
#pragma unroll
      for (int q = 0; q < NF; ++q) {
        st(u.p[q], p4 + at * NF + q);
        st(u.m[q], m4 + at * NF + q);
        if constexpr (ADAM) st(u.v[q], v4 + at * NF + q);
      }
    }
    if constexpr (SHADOW) st(Elt<bf16_t>::pack(pn), h4 + at);
  };
  const int64_t stride = int64_t(kBlock) * gridDim.y;
  int64_t i = int64_t(blockIdx.y) * kBlock + threadIdx.x;
  for (; i + stride < nv; i += 2 * stride) {
    Unit u0 = load(i), u1 = load(i + stride);
    update(u0, i);
    update(u1, i + stride);
  }
  for (; i < nv; i += stride) {
    Unit u = load(i);
    update(u, i);
  }
}

// The end of the kernel arguments: the rounding seed alone, or the group table
// in front of it.  The seed is the last member in both, so the arguments keep
// one layout whichever tail the kernel takes.
struct PlainTail {
  uint32_t seed;
};
// The flat buffer is cut into segments (seg_end: ascending exclusive ends, the
// last one S; seg_group: each segment's group) and rows[g] = {neg_lr, wd, lr,
// decay} holds group g's host-rounded scalars in DEVICE memory, read when the
// kernel runs: rewriting the rows between the replays of a captured step
// changes its learning rate.
struct GroupTail {
  const int64_t* __restrict__ seg_end;
  const int32_t* __restrict__ seg_group;
  const float4* __restrict__ rows;
  int32_t nseg, G;
  uint32_t seed;
};
// LAMB's: the group table with one trust ratio per segment behind it (the ratio
// kernel's table); a segment is one layer.
struct LambTail {
  const int64_t* __restrict__ seg_end;
  const int32_t* __restrict__ seg_group;
  const float4* __restrict__ rows;
  int32_t nseg, G;
  const float* __restrict__ trust;
  uint32_t seed;
};

// Region walk spelled out here as in count_mean, on purpose (the comment at
// count_mean_kernel, counts.hip).  Tail = PlainTail: one set of scalars for the
// whole buffer, from k.  Tail = GroupTail: a region is walked by its
// intersections with the segments, each processed as the plain pass processes a
// region, with its group's row.  Everything that picks the segment and the row
// is wave-uniform (scalar loads, scalar branches).
template <typename TS, typename TM, typename TP, int KIND, bool SHADOW, bool NT, typename Tail>
__global__ __launch_bounds__(kBlock) void count_optim_kernel(TP* __restrict__ p, TM* __restrict__ m,
                                                             TM* __restrict__ v, bf16_t* __restrict__ shadow,
                                                             const TS* __restrict__ src,
                                                             const int32_t* __restrict__ counts, int64_t S,
                                                             int64_t step, int32_t N, int64_t C, int32_t kmax,
                                                             OptimK k, const int32_t* __restrict__ t,
                                                             const float* __restrict__ sq,
                                                             const int32_t* __restrict__ guard, Tail tail) {
  constexpr bool GROUPS = std::is_same_v<Tail, GroupTail> || std::is_same_v<Tail, LambTail>;
  static_assert((KIND == kLamb) == std::is_same_v<Tail, LambTail>, "LAMB, and LAMB alone, takes the trust table");
  static_assert(!(GROUPS && NT), "the grouped pass has no nontemporal variant");
  // a skipped step (the norm pass's verdict, below at count_sqnorm_kernel): wave-uniform, in every workgroup,
  // before t, sq or anything else is read -- nothing is loaded and nothing is stored
  if (guard && guard[0] == 0) return;
  const StepCoef sc = step_coefficients<KIND>(k, t, sq);
  Coef c{};
  if constexpr (!GROUPS) c = lr_coefficients<KIND>(sc, k.lr, k.eps);
  uint32_t key = 0;
  if constexpr (Elt<TM>::kPerVec == 8) key = sr_key(tail.seed, t);
  const int64_t nregions = int64_t(N) * kmax;
  for (int64_t reg = blockIdx.x; reg < nregions; reg += gridDim.x) {
    const int32_t j = int32_t(reg / kmax);
    const int64_t kk = reg - int64_t(j) * kmax;
    const int64_t bs = j * step < S ? j * step : S;
    const int64_t be = j >= N - 1 ? S : ((j + 1) * step < S ? (j + 1) * step : S);
    const int64_t s = bs + kk * C;
    if (s >= be) continue;
    const int64_t e = s + C < be ? s + C : be;
    const int32_t cnt = counts[reg];
    if (cnt <= 0) continue;  // missing: nothing of this region is loaded or stored
    const float fv = float(cnt);
    if constexpr (GROUPS) {
      // the first segment whose end is past s (there is one: the last segment ends at S > s)
      int32_t lo = 0, hi = tail.nseg - 1;
      while (lo < hi) {
        const int32_t mid = (lo + hi) >> 1;
        if (tail.seg_end[mid] > s) hi = mid;
        else lo = mid + 1;
      }
      int64_t cur = s;
      for (int32_t si = lo; cur < e && si < tail.nseg; ++si) {
        const int64_t se = tail.seg_end[si];
        const int64_t ee = se < e ? se : e;
        if (ee <= cur) continue;
        const uint32_t g = uint32_t(tail.seg_group[si]);
        if (g < uint32_t(tail.G)) {  // the launcher checked the host copy; a row is never read out of bounds
          const float4 r = tail.rows[g];
          OptimK kg = k;
          kg.neg_lr = r.x;
          kg.wd = r.y;
          kg.lr = r.z;
          kg.decay = r.w;
          float tr = 1.f;
          if constexpr (KIND == kLamb) tr = tail.trust[si];
          update_range<TS, TM, TP, KIND, SHADOW, false, true>(p, m, v, shadow, src, cur, ee, fv, kg,
                                                              lr_coefficients<KIND>(sc, r.z, k.eps, tr), key);
        }
        cur = ee;
      }
    } else {
      update_range<TS, TM, TP, KIND, SHADOW, NT>(p, m, v, shadow, src, s, e, fv, k, c, key);
    }
  }
}

// Sum over the workgroup in a fixed order: xor tree in the wave, waves in order.
__device__ __forceinline__ float block_sum(float x, float* red) {
  for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
  __syncthreads();  // red may still be read by a previous sum
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
  __syncthreads();
  float r = red[0];
  for (int w = 1; w < kBlock / 64; ++w) r += red[w];
  return r;
}

constexpr int kSqUnroll = 4;

template <typename TS>
__global__ __launch_bounds__(kBlock) void count_sqnorm_kernel(float* __restrict__ sq, const TS* __restrict__ src,
                                                              const int32_t* __restrict__ counts, int64_t S,
                                                              int64_t step, int32_t N, int64_t C, int32_t kmax,
                                                              float* __restrict__ part,
                                                              uint32_t* __restrict__ ticket,
                                                              int32_t* __restrict__ guard, int32_t* __restrict__ t) {
  constexpr int E = Elt<TS>::kPerVec;
  __shared__ float red[kBlock / 64 + 1];
  float acc = 0.f;
  const int64_t nregions = int64_t(N) * kmax;
  for (int64_t reg = blockIdx.x; reg < nregions; reg += gridDim.x) {
    const int32_t j = int32_t(reg / kmax);
    const int64_t kk = reg - int64_t(j) * kmax;
    const int64_t bs = j * step < S ? j * step : S;
    const int64_t be = j >= N - 1 ? S : ((j + 1) * step < S ? (j + 1) * step : S);
    const int64_t s = bs + kk * C;
    if (s >= be) continue;
    const int64_t e = s + C < be ? s + C : be;
    const int32_t cnt = counts[reg];
    if (cnt <= 0) continue;
    const float fv = float(cnt);
    int64_t a = (s + E - 1) & ~int64_t(E - 1);
    if (a > e) a = e;
    const int64_t nv = (e - a) / E;
    auto one = [&](int64_t i) {
      const float g = Elt<TS>::to_f(src[i]) / fv;
      acc += g * g;
    };
    if (blockIdx.y == 0) {
      for (int64_t i = s + threadIdx.x; i < a; i += kBlock) one(i);
      for (int64_t i = a + nv * E + threadIdx.x; i < e; i += kBlock) one(i);
    }
    const v4u* s4 = reinterpret_cast<const v4u*>(src + a);
    auto vec = [&](const v4u& sv) {
      float g[E];
#pragma unroll
      for (int q = 0; q < E; ++q) g[q] = 0.f;
      Elt<TS>::add(g, sv);
#pragma unroll
      for (int q = 0; q < E; ++q) {
        const float x = g[q] / fv;
        acc += x * x;
      }
    };
    constexpr int U = kSqUnroll;
    const int64_t stride = int64_t(kBlock) * gridDim.y;
    int64_t i = int64_t(blockIdx.y) * kBlock + threadIdx.x;
    for (; i + (U - 1) * stride < nv; i += U * stride) {
      v4u sv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) sv[u] = s4[i + u * stride];
#pragma unroll
      for (int u = 0; u < U; ++u) vec(sv[u]);
    }
    for (; i < nv; i += stride) vec(s4[i]);
  }
  acc = block_sum(acc, red);
  const uint32_t nwg = gridDim.x * gridDim.y, wg = blockIdx.y * gridDim.x + blockIdx.x;
  const auto rs = xgmi::sys_rsrc(part, int64_t(nwg) * 4);
  if (threadIdx.x == 0) {
    // the workgroup's partial, written through for the last arriver
    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(acc), rs, int(wg * 4), 0, xgmi::kSysAux);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    red[kBlock / 64] =
        __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == nwg - 1 ? 1.f : 0.f;
  }
  __syncthreads();
  if (red[kBlock / 64] == 0.f) return;
  // last workgroup: the partials in index order per thread, then the fixed tree
  float sum = 0.f;
  for (uint32_t i = threadIdx.x; i < nwg; i += kBlock)
    sum += __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, int(i * 4), 0, xgmi::kSysAux));
  sum = block_sum(sum, red);
  if (threadIdx.x == 0) {
    sq[0] = sum;
    __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // re-armed for the next launch
    if (guard) {
      // the verdict: the step is applied iff the sum is a finite fp32 number (its exponent bits are not all
      // ones).  This thread alone reads and writes the record and the step; the update pass behind this
      // kernel on the stream sees both across the kernel boundary.
      if ((__float_as_uint(sum) & 0x7f800000u) != 0x7f800000u) {
        guard[0] = 1;
        guard[2] = 0;
        *t += 1;
      } else {
        guard[0] = 0;
        guard[1] += 1;
        guard[2] += 1;
      }
    }
  }
}

// LAMB's norm pass (the file header: "LAMB").  The flat buffer is cut into tiles
// of kLambTile elements (a multiple of the 8-element unit, so a unit never
// crosses a tile's end); one workgroup takes a tile at a time.  A tile is walked
// by its intersections with the layers (the segments, found as the grouped pass
// finds them), a piece by its intersections with the count regions, whose index
// comes from the geometry arithmetic; a region with count 0 is skipped before
// any load.  Everything that picks layer, region and count is wave-uniform.
// Per element m_new, v_new and u come from lamb_u in registers; nothing but the
// partials is written.  The sums of p^2 and u^2 of a piece go to slot tile +
// layer: along the pieces either index grows, so no slot is shared, and a
// layer's pieces are the consecutive slots [first tile + layer, last tile +
// layer].  Every slot a layer owns is written by every launch (zeros for a piece
// with no contributor).  A piece's sum depends on the piece alone -- per thread:
// head, tail, then its units in ascending order; then block_sum -- never on the
// grid.
constexpr int kLambTile = 8192;
static_assert(kLambTile % 8 == 0, "a unit must not cross a tile's end");

template <typename TS, typename TM, typename TP>
__device__ __forceinline__ void norm_range(const TP* __restrict__ p, const TM* __restrict__ m,
                                           const TM* __restrict__ v, const TS* __restrict__ src, int64_t s,
                                           int64_t e, float fv, const OptimK& k, const Coef& c, float& pp, float& uu) {
#pragma clang fp contract(off)
  constexpr int E = 8;
  constexpr int ES = Elt<TS>::kPerVec;
  constexpr int NS = E / ES;
  constexpr int NF = E / Elt<float>::kPerVec;
  constexpr int NM = E / Elt<TM>::kPerVec;
  constexpr int NP = E / Elt<TP>::kPerVec;  // bf16 parameters are read widened, as the update reads them
  static_assert(NP == NF || NM == 1, "bf16 parameters: bf16 moments");
  int64_t a = (s + E - 1) & ~int64_t(E - 1);
  if (a > e) a = e;
  const int64_t nv = (e - a) / E;
  auto acc = [&](float g, float pi, float mi, float vi) {
    const float u = lamb_u(g / fv, pi, mi, vi, k, c);
    pp = pp + pi * pi;
    uu = uu + u * u;
  };
  auto one = [&](int64_t i) {
    acc(Elt<TS>::to_f(src[i]), Elt<TP>::to_f(p[i]), Elt<TM>::to_f(m[i]), Elt<TM>::to_f(v[i]));
  };
  for (int64_t i = s + threadIdx.x; i < a; i += kBlock) one(i);
  for (int64_t i = a + nv * E + threadIdx.x; i < e; i += kBlock) one(i);
  const v4u* s4 = reinterpret_cast<const v4u*>(src + a);
  const v4u* p4 = reinterpret_cast<const v4u*>(p + a);
  const v4u* m4 = reinterpret_cast<const v4u*>(m + a);
  const v4u* v4 = reinterpret_cast<const v4u*>(v + a);
  struct Unit {
    v4u s[NS], p[NP], m[NM], v[NM];
  };
  auto load = [&](int64_t at) {
    Unit u;
#pragma unroll
    for (int q = 0; q < NS; ++q) u.s[q] = s4[at * NS + q];
#pragma unroll
    for (int q = 0; q < NP; ++q) u.p[q] = p4[at * NP + q];
#pragma unroll
    for (int q = 0; q < NM; ++q) u.m[q] = m4[at * NM + q];
#pragma unroll
    for (int q = 0; q < NM; ++q) u.v[q] = v4[at * NM + q];
    return u;
  };
  auto sum = [&](const Unit& u) {
    float g[E];
#pragma unroll
    for (int q = 0; q < E; ++q) g[q] = 0.f;
#pragma unroll
    for (int q = 0; q < NS; ++q) Elt<TS>::add(reinterpret_cast<float(&)[ES]>(g[q * ES]), u.s[q]);
#pragma unroll
    for (int q = 0; q < E; ++q)
      acc(g[q], unit_elem<TP>(u.p, q), unit_elem<TM>(u.m, q), unit_elem<TM>(u.v, q));
  };
  int64_t i = threadIdx.x;
  for (; i + kBlock < nv; i += 2 * kBlock) {
    const Unit u0 = load(i), u1 = load(i + kBlock);
    sum(u0);
    sum(u1);
  }
  for (; i < nv; i += kBlock) sum(load(i));
}

template <typename TS, typename TM, typename TP>
__global__ __launch_bounds__(kBlock) void lamb_norms_kernel(float2* __restrict__ part, const TP* __restrict__ p,
                                                            const TM* __restrict__ m, const TM* __restrict__ v,
                                                            const TS* __restrict__ src,
                                                            const int32_t* __restrict__ counts, int64_t S,
                                                            int64_t step, int32_t N, int64_t C, int32_t kmax,
                                                            OptimK k, const int32_t* __restrict__ t,
                                                            const float* __restrict__ sq,
                                                            const int32_t* __restrict__ guard,
                                                            const int64_t* __restrict__ seg_end,
                                                            const int32_t* __restrict__ seg_group,
                                                            const float4* __restrict__ rows, int32_t nseg, int32_t G) {
  __shared__ float red[kBlock / 64];
  if (guard && guard[0] == 0) return;  // a skipped step: the partials and the trust table keep what they hold
  const StepCoef sc = step_coefficients<kLamb>(k, t, sq);
  const Coef c = lr_coefficients<kLamb>(sc, 0.f, k.eps);  // the step size is the update pass's business
  const int64_t ntiles = (S + kLambTile - 1) / kLambTile;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t ts = tile * kLambTile;
    const int64_t te = ts + kLambTile < S ? ts + kLambTile : S;
    // the first layer whose end is past ts (there is one: the last layer ends at S > ts)
    int32_t lo = 0, hi = nseg - 1;
    while (lo < hi) {
      const int32_t mid = (lo + hi) >> 1;
      if (seg_end[mid] > ts) hi = mid;
      else lo = mid + 1;
    }
    int64_t cur = ts;
    for (int32_t li = lo; cur < te && li < nseg; ++li) {
      const int64_t se = seg_end[li];
      const int64_t pe = se < te ? se : te;
      if (pe <= cur) continue;
      float pp = 0.f, uu = 0.f;
      const uint32_t g = uint32_t(seg_group[li]);
      if (g < uint32_t(G)) {  // as in count_optim: a row is never read out of bounds
        OptimK kg = k;
        kg.wd = rows[g].y;
        for (int64_t x = cur; x < pe;) {
          // the count region of x: block j, chunk kk of it
          const int64_t jj = step > 0 ? x / step : int64_t(N - 1);
          const int64_t j = jj < N - 1 ? jj : int64_t(N - 1);
          const int64_t bs = j * step;
          const int64_t be = j >= N - 1 ? S : ((j + 1) * step < S ? (j + 1) * step : S);
          const int64_t kk = (x - bs) / C;
          int64_t ee = bs + (kk + 1) * C;
          if (ee > be) ee = be;
          if (ee > pe) ee = pe;
          if (ee <= x) ee = pe;  // not with a consistent geometry; the walk must advance
          // a chunk past kmax has no count: missing, as for the region walks, which never visit it
          const int32_t cnt = kk < kmax ? counts[j * kmax + kk] : 0;
          if (cnt > 0) norm_range<TS, TM, TP>(p, m, v, src, x, ee, float(cnt), kg, c, pp, uu);
          x = ee;
        }
      }
      pp = block_sum(pp, red);
      uu = block_sum(uu, red);
      if (threadIdx.x == 0) part[tile + li] = make_float2(pp, uu);
      cur = pe;
    }
  }
}

// One workgroup per layer: the layer's partials in slot order per thread, then
// the fixed tree, then r = ||p|| / ||u|| where both squared sums are positive
// finite numbers, else 1; 1 as well for a layer whose adapt flag is 0.
__global__ __launch_bounds__(kBlock) void lamb_trust_kernel(float* __restrict__ trust,
                                                            const float2* __restrict__ part,
                                                            const int64_t* __restrict__ seg_end,
                                                            const int32_t* __restrict__ adapt, int32_t nseg,
                                                            const int32_t* __restrict__ guard) {
#pragma clang fp contract(off)
  __shared__ float red[kBlock / 64];
  if (guard && guard[0] == 0) return;
  const int32_t li = blockIdx.x;
  if (li >= nseg) return;
  if (adapt[li] == 0) {  // wave-uniform: nothing of the partials is read
    if (threadIdx.x == 0) trust[li] = 1.f;
    return;
  }
  const int64_t ls = li > 0 ? seg_end[li - 1] : 0, le = seg_end[li];
  float pp = 0.f, uu = 0.f;
  if (le > ls) {
    const int64_t first = ls / kLambTile + li, last = (le - 1) / kLambTile + li;
    for (int64_t i = first + threadIdx.x; i <= last; i += kBlock) {
      const float2 x = part[i];
      pp = pp + x.x;
      uu = uu + x.y;
    }
  }
  pp = block_sum(pp, red);
  uu = block_sum(uu, red);
  if (threadIdx.x == 0) {
    const bool ok = pp > 0.f && uu > 0.f && (__float_as_uint(pp) & 0x7f800000u) != 0x7f800000u &&
                    (__float_as_uint(uu) & 0x7f800000u) != 0x7f800000u;
    trust[li] = ok ? sqrtf(pp) / sqrtf(uu) : 1.f;
  }
}

bool aligned16(const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; }

// Run-time values as template arguments, in the style of dispatch_int:
// f(Elem<float>{}) or f(Elem<bf16_t>{}) for a dtype, f(std::bool_constant<b>{}) for a flag.
template <typename T>
struct Elem {
  using type = T;
};
template <typename F>
void with_elem(DType dt, F&& f) {
  if (dt == DType::BF16) f(Elem<bf16_t>{});
  else f(Elem<float>{});
}
template <typename F>
void with_flag(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}
template <typename F>
void with_kind(OptimKind kind, F&& f) {
  if (kind == OptimKind::LAMB) f(std::integral_constant<int, kLamb>{});
  else if (kind == OptimKind::AdamW) f(std::integral_constant<int, kAdam>{});
  else f(std::integral_constant<int, kSGD>{});
}

// The host copies of the segment tables against the buffer's size (the kernels trust the device copies).
void check_groups(const OptimGroups& g, int64_t S, const std::string& who) {
  AKKA_CHECK(g.nseg > 0 && g.ngroups > 0 && g.seg_end && g.seg_group && g.rows && g.host_seg_end &&
                 g.host_seg_group,
             who + ": no segments, no groups or a null table");
  AKKA_CHECK(aligned16(g.rows) && (reinterpret_cast<uintptr_t>(g.seg_end) & 7) == 0 &&
                 (reinterpret_cast<uintptr_t>(g.seg_group) & 3) == 0,
             who + ": the rows must be 16-B aligned, the segment tables naturally");
  int64_t prev = 0;
  for (int32_t i = 0; i < g.nseg; ++i) {
    AKKA_CHECK(g.host_seg_end[i] > prev, who + ": segment ends must be positive and ascending");
    AKKA_CHECK(g.host_seg_group[i] >= 0 && g.host_seg_group[i] < g.ngroups,
               who + ": a segment's group is outside [0, groups)");
    prev = g.host_seg_end[i];
  }
  AKKA_CHECK(prev == S, who + ": the last segment must end at the buffer's size");
}

// with groups the learning rate and the decay come from the rows (o's are 0 then)
OptimK host_scalars(const OptimSpec& o) {
  OptimK k{};
  k.neg_lr = float(-o.lr);
  k.wd = float(o.weight_decay);
  k.mu = float(o.momentum);
  k.nesterov = o.nesterov ? 1 : 0;
  k.lr = float(o.lr);
  k.decay = float(1.0 - o.lr * o.weight_decay);
  k.b1 = float(o.beta1);
  k.w1 = float(1.0 - o.beta1);
  k.b2 = float(o.beta2);
  k.w2 = float(1.0 - o.beta2);
  k.eps = float(o.eps);
  k.max_norm = float(o.max_norm);
  return k;
}

int64_t lamb_tiles(int64_t S) { return (S + kLambTile - 1) / kLambTile; }

}  // namespace

void launch_count_optim(hipStream_t s, const OptimBuffers& b, const CountsTable& ct, const OptimSpec& o,
                        const OptimGroups* groups, bool nt) {
  if (ct.S <= 0) return;
  const bool lamb = o.kind == OptimKind::LAMB;
  const bool adam = o.kind == OptimKind::AdamW || lamb;  // a second moment and the step
  const bool bf_state = b.state_dt == DType::BF16;
  AKKA_CHECK(!(bf_state && nt), "count_optim: no nontemporal variant with bfloat16 state");
  AKKA_CHECK(!(groups && nt), "count_optim: no nontemporal variant with parameter groups");
  const bool bf_param = b.param_dt == DType::BF16;
  AKKA_CHECK(!bf_param || bf_state, "count_optim: bfloat16 parameters need bfloat16 state");
  AKKA_CHECK(!(bf_param && b.shadow), "count_optim: no shadow with bfloat16 parameters (they are the bf16 weights)");
  AKKA_CHECK(!(bf_param && nt), "count_optim: no nontemporal variant with bfloat16 parameters");
  AKKA_CHECK(!lamb || (groups && groups->trust), "count_optim: LAMB needs groups, one segment per layer, with a "
                                                 "trust table");
  // bf16 state reads the step for its rounding key, whatever the kind
  AKKA_CHECK(b.p && b.m && b.src && ct.counts && (!adam || (b.v && b.t)) && (!bf_state || b.t),
             "count_optim: null buffer");
  AKKA_CHECK(!b.guard || (b.sq && b.t), "count_optim: a guard needs the norm pass's sq and the step t");
  AKKA_CHECK(aligned16(b.p) && aligned16(b.m) && aligned16(b.v) && aligned16(b.shadow) && aligned16(b.src),
             "count_optim: buffers must be 16-B aligned");
  ct.check("count_optim");
  if (groups) check_groups(*groups, ct.S, "count_optim");
  const OptimK k = host_scalars(o);
  const RegionGrid rg = region_grid(ct.regions(), ct.S, kMaxGrid);
  with_elem(b.src_dt, [&](auto ts) {
    with_kind(o.kind, [&](auto kd) {
      with_flag(b.shadow != nullptr, [&](auto sh) {
        auto launch_p = [&](auto tp, auto tm, auto ntv, auto tail) {
          using TS = typename decltype(ts)::type;
          using TM = typename decltype(tm)::type;
          using TP = typename decltype(tp)::type;
          constexpr int KIND = decltype(kd)::value;
          constexpr bool SH = decltype(sh)::value, NTV = decltype(ntv)::value;
          // LAMB takes its own tail, the other kinds theirs: the mixed instantiations do not exist; nor do those
          // of bf16 parameters with fp32 moments, a shadow or nontemporal accesses (refused above)
          constexpr bool param_ok = std::is_same_v<TP, float> || (std::is_same_v<TM, bf16_t> && !SH && !NTV);
          if constexpr ((KIND == kLamb) == std::is_same_v<decltype(tail), LambTail> && param_ok)
            hipLaunchKernelGGL((count_optim_kernel<TS, TM, TP, KIND, SH, NTV, decltype(tail)>),
                               dim3(rg.grid, rg.split), dim3(kBlock), 0, s, static_cast<TP*>(b.p),
                               static_cast<TM*>(b.m), static_cast<TM*>(b.v), static_cast<bf16_t*>(b.shadow),
                               static_cast<const TS*>(b.src), ct.counts, ct.S, ct.step, ct.N, ct.C, ct.kmax, k, b.t,
                               b.sq, b.guard, tail);
        };
        auto launch = [&](auto tm, auto ntv, auto tail) {
          with_elem(b.param_dt, [&](auto tp) { launch_p(tp, tm, ntv, tail); });
        };
        // nontemporal accesses: fp32 state without groups only (checked above)
        if (nt) return launch(Elem<float>{}, std::true_type{}, PlainTail{b.seed});
        with_elem(b.state_dt, [&](auto tm) {
          if (lamb)
            launch(tm, std::false_type{},
                   LambTail{groups->seg_end, groups->seg_group, reinterpret_cast<const float4*>(groups->rows),
                            groups->nseg, groups->ngroups, groups->trust, b.seed});
          else if (groups)
            launch(tm, std::false_type{},
                   GroupTail{groups->seg_end, groups->seg_group, reinterpret_cast<const float4*>(groups->rows),
                             groups->nseg, groups->ngroups, b.seed});
          else launch(tm, std::false_type{}, PlainTail{b.seed});
        });
      });
    });
  });
  check_launch("count_optim");
}

int32_t count_sqnorm_partials() { return kMaxGrid; }

void launch_count_sqnorm(hipStream_t s, float* sq, const void* src, DType src_dt, const CountsTable& ct, float* part,
                         uint32_t* ticket, int32_t* guard, int32_t* t) {
  if (ct.S <= 0) return;
  AKKA_CHECK(sq && src && ct.counts && part && ticket, "count_sqnorm: null buffer");
  AKKA_CHECK((guard != nullptr) == (t != nullptr), "count_sqnorm: a guard and a writable step t, both or neither");
  AKKA_CHECK(aligned16(src), "count_sqnorm: the sum must be 16-B aligned");
  ct.check("count_sqnorm");
  // grid * split <= kMaxGrid: one partial each in `part`
  const auto [grid, split] = region_grid(ct.regions(), ct.S, kMaxGrid);
  // plain loads: the update pass reads the sum next
#define AKKA_SQ(TS)                                                                                          \
  hipLaunchKernelGGL((count_sqnorm_kernel<TS>), dim3(grid, split), dim3(kBlock), 0, s, sq,                   \
                     static_cast<const TS*>(src), ct.counts, ct.S, ct.step, ct.N, ct.C, ct.kmax, part, ticket, \
                     guard, t)
  if (src_dt == DType::BF16) AKKA_SQ(bf16_t);
  else AKKA_SQ(float);
#undef AKKA_SQ
  check_launch("count_sqnorm");
}

int32_t lamb_tile() { return kLambTile; }

void launch_lamb_norms(hipStream_t s, const OptimBuffers& b, const CountsTable& ct, const OptimSpec& o,
                       const OptimGroups& groups, float* part, int64_t slots, int32_t grid) {
  if (ct.S <= 0) return;
  AKKA_CHECK(b.p && b.m && b.v && b.t && b.src && ct.counts && part, "lamb_norms: null buffer");
  AKKA_CHECK(!b.guard || b.sq, "lamb_norms: a guard needs the norm pass's sq");
  AKKA_CHECK(b.param_dt != DType::BF16 || b.state_dt == DType::BF16,
             "lamb_norms: bfloat16 parameters need bfloat16 state");
  AKKA_CHECK(aligned16(b.p) && aligned16(b.m) && aligned16(b.v) && aligned16(b.src) &&
                 (reinterpret_cast<uintptr_t>(part) & 7) == 0,
             "lamb_norms: buffers must be 16-B aligned, the partials 8-B");
  ct.check("lamb_norms");
  AKKA_CHECK(ct.N > 0 && ct.kmax > 0, "lamb_norms: bad geometry");
  check_groups(groups, ct.S, "lamb_norms");
  const int64_t ntiles = lamb_tiles(ct.S);
  // the last piece writes slot (ntiles - 1) + (nseg - 1)
  AKKA_CHECK(slots >= ntiles + groups.nseg, "lamb_norms: the workspace needs tiles + layers slots");
  AKKA_CHECK(grid >= 0, "lamb_norms: grid is >= 0 (0: the launcher's choice)");
  // any grid gives the same bits: a piece's sum does not depend on which workgroup computed it
  int64_t g = grid > 0 ? grid : ntiles;
  if (g > kMaxGrid) g = kMaxGrid;
  if (g > ntiles) g = ntiles;
  const OptimK k = host_scalars(o);
  with_elem(b.src_dt, [&](auto ts) {
    with_elem(b.state_dt, [&](auto tm) {
      with_elem(b.param_dt, [&](auto tp) {
        using TS = typename decltype(ts)::type;
        using TM = typename decltype(tm)::type;
        using TP = typename decltype(tp)::type;
        // bf16 parameters with fp32 moments: refused above, not instantiated
        if constexpr (std::is_same_v<TP, float> || std::is_same_v<TM, bf16_t>)
          hipLaunchKernelGGL((lamb_norms_kernel<TS, TM, TP>), dim3(int(g)), dim3(kBlock), 0, s,
                             reinterpret_cast<float2*>(part), static_cast<const TP*>(b.p),
                             static_cast<const TM*>(b.m), static_cast<const TM*>(b.v), static_cast<const TS*>(b.src),
                             ct.counts, ct.S, ct.step, ct.N, ct.C, ct.kmax, k, b.t, b.sq, b.guard, groups.seg_end,
                             groups.seg_group, reinterpret_cast<const float4*>(groups.rows), groups.nseg,
                             groups.ngroups);
      });
    });
  });
  check_launch("lamb_norms");
}

void launch_lamb_trust(hipStream_t s, float* trust, const float* part, int64_t slots, const OptimGroups& groups,
                       int64_t S, const int32_t* adapt, const int32_t* guard) {
  if (S <= 0) return;
  AKKA_CHECK(trust && part && adapt && (reinterpret_cast<uintptr_t>(part) & 7) == 0, "lamb_trust: null buffer");
  check_groups(groups, S, "lamb_trust");
  AKKA_CHECK(slots >= lamb_tiles(S) + groups.nseg, "lamb_trust: the workspace needs tiles + layers slots");
  hipLaunchKernelGGL(lamb_trust_kernel, dim3(groups.nseg), dim3(kBlock), 0, s, trust,
                     reinterpret_cast<const float2*>(part), groups.seg_end, adapt, groups.nseg, guard);
  check_launch("lamb_trust");
}

}  // namespace akka
