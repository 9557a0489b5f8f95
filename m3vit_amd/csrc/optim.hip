// The optimizer tail of a training step: gradient unscale, global-norm clip, overflow skip and the AdamW / Adam / SGD update
// of every parameter tensor in three launches (m3_optim_prepare: per-chunk norm partials + a one-workgroup finalize;
// m3_optim_step: one pass over p, g, m, v).  One workgroup per 4096-element chunk of one tensor, found by a binary search over
// the device-resident descriptor table (as m3_cast_batch).  No atomics; every sum has a fixed order, so results are the same
// bits from run to run.
#include "reduce_dev.h"
#include <math.h>

namespace m3 {

constexpr int OPT_CHUNK = M3_OPTIM_CHUNK;      // elements per workgroup: 256 threads x 4 floats x 4 pieces
constexpr int OPT_PIECES = 4;
constexpr int OPT_HEAD = 8;                    // floats of the state header; 8 derived doubles per group follow

struct OptimDesc {           // = m3_optim_desc
  float *p; const float *g; float *m; float *v;
  int64_t n;
  int32_t group, chunk_start, vec_ok;
};

struct OptimState {          // the first OPT_HEAD floats of `state`
  int32_t skip, step;
  float total_norm, clip_coef, inv_scale;
  float gscale;              // inv_scale * clip_coef: the one factor the step kernel applies to a gradient
  float pad[2];
};

// per group, written by the finalize kernel: everything the step kernel needs.  Doubles: a coefficient rounded to fp32 costs
// half an ulp of the update each, and the bound the step is held to (4 ulp of |p| + lr per step) has no room for five of them
struct OptimCoef {
  double step_size;          // Adam: lr / (1 - beta1^t); SGD: lr
  double c1;                 // Adam: 1 / sqrt(1 - beta2^t); SGD: momentum
  double decay_mul;          // decoupled decay: 1 - lr * wd, else 1
  double l2;                 // weight decay added to the gradient, else 0
  double omb1, beta2, omb2;  // Adam: 1 - beta1, beta2, 1 - beta2
  double eps_or_nesterov;    // Adam: eps; SGD: 1 when nesterov
};

__device__ __forceinline__ OptimDesc find_desc(const OptimDesc *__restrict__ descs, int n_desc, int b) {
  int lo = 0, hi = n_desc - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (descs[mid].chunk_start <= b) lo = mid; else hi = mid - 1;
  }
  return descs[lo];
}

__device__ __forceinline__ uint32_t non_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) == 0x7f800000u; }

// ------------------------------------------------------------------------------------------------ norm partials
__global__ __launch_bounds__(256) void optim_norm_kernel(const OptimDesc *__restrict__ descs, int n_desc, int total_chunks,
                                                         float *__restrict__ partials) {
  __shared__ uint32_t s_bad[4];
  const int b = blockIdx.x, t = threadIdx.x;
  const OptimDesc d = find_desc(descs, n_desc, b);
  const int64_t base = (int64_t)(b - d.chunk_start) * OPT_CHUNK;
  const int64_t n4 = d.n & ~(int64_t)3;
  const float *g = d.g + base;
  float acc = 0.f;
  uint32_t bad = 0;
  if (d.vec_ok && n4 > 0) {
    const int64_t left = n4 - base;                                   // whole float4s of this chunk hold elements [0, left)
    const int valid = (int)(left < OPT_CHUNK ? left : OPT_CHUNK);
    f32x4 x[OPT_PIECES];
#pragma unroll
    for (int k = 0; k < OPT_PIECES; ++k) {
      const int e = (k * 256 + t) * 4;
      x[k] = *(const f32x4 *)(g + (e < valid ? e : valid - 4));       // clamped, never predicated: all loads issue at once
    }
#pragma unroll
    for (int k = 0; k < OPT_PIECES; ++k) {
      const bool on = (k * 256 + t) * 4 < valid;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float e = on ? x[k][j] : 0.f;
        acc = __builtin_fmaf(e, e, acc);
        bad |= non_finite(e);
      }
    }
    const int64_t i = n4 + t;                                         // the up to 3 elements behind the last whole float4
    if (base + OPT_CHUNK >= d.n && i < d.n) {
      const float e = d.g[i];
      acc = __builtin_fmaf(e, e, acc);
      bad |= non_finite(e);
    }
  } else {
#pragma unroll 4
    for (int k = 0; k < OPT_PIECES * 4; ++k) {
      const int64_t i = base + k * 256 + t;
      if (i < d.n) {
        const float e = d.g[i];
        acc = __builtin_fmaf(e, e, acc);
        bad |= non_finite(e);
      }
    }
  }
  bad = __any((int)bad) ? 1u : 0u;
  if ((t & 63) == 0) s_bad[t >> 6] = bad;
  block_partials<1>({acc}, partials);              // row 0 of [2][total_chunks]; its barrier also stands between s_bad's writes and reads
  if (t == 0) partials[total_chunks + b] = (s_bad[0] | s_bad[1] | s_bad[2] | s_bad[3]) ? 1.f : 0.f;
}

// ----------------------------------------------------------------------------------------------------- finalize
// one workgroup: the global norm, the clip coefficient, the skip decision, the step counter and every group's coefficients
__global__ __launch_bounds__(256) void optim_finalize_kernel(const float *__restrict__ partials, int n_part,
                                                             const float *__restrict__ hyper, int n_groups, int kind,
                                                             const float *__restrict__ grad_scale,
                                                             const float *__restrict__ found_inf_in, float max_norm,
                                                             float *__restrict__ state) {
  __shared__ int s_skip, s_step;
  const int t = threadIdx.x;
  // both rows as sums: the flags are 1.f or 0.f, so their sum (exact in double) is non-zero where their or is
  const Totals<2, 0> tot = reduce_partials<2, 0>(partials, n_part, n_part);
  if (t == 0) {
    const double sum = tot.s[0];
    int any = tot.s[1] != 0.0;
    OptimState *st = (OptimState *)state;
    const float inv_scale = grad_scale ? 1.0f / *grad_scale : 1.0f;
    if (found_inf_in && *found_inf_in != 0.f) any = 1;
    const float total_norm = (float)(sqrt(sum) * (double)inv_scale);
    float clip = 1.0f;
    if (max_norm > 0.f) clip = fminf(1.0f, max_norm / (total_norm + 1e-6f));      // torch.nn.utils.clip_grad_norm_
    const int step = st->step + (any ? 0 : 1);                                     // a skipped step does not count
    st->skip = any;
    st->step = step;
    st->total_norm = total_norm;
    st->clip_coef = clip;
    st->inv_scale = inv_scale;
    st->gscale = inv_scale * clip;
    s_skip = any;
    s_step = step;
  }
  __syncthreads();
  if (s_skip) return;                              // the step kernel returns before it reads a coefficient
  const double step = (double)s_step;
  for (int gi = t; gi < n_groups; gi += 256) {
    const float *h = hyper + (int64_t)gi * M3_OPTIM_HYPER;
    OptimCoef *c = (OptimCoef *)(state + OPT_HEAD) + gi;
    const double lr = h[0], wd = h[4];
    const double b1 = (double)h[1] + (double)h[6], b2 = (double)h[2] + (double)h[7];   // hi + lo: the host's doubles
    const int flags = (int)h[5];
    const bool decoupled = flags & M3_OPTIM_DECOUPLED;
    c->decay_mul = decoupled ? 1.0 - lr * wd : 1.0;
    c->l2 = decoupled ? 0.0 : wd;
    if (kind == M3_OPTIM_SGD) {
      c->step_size = lr;
      c->c1 = h[1];
      c->omb1 = c->beta2 = c->omb2 = 0.0;
      c->eps_or_nesterov = (flags & M3_OPTIM_NESTEROV) ? 1.0 : 0.0;
    } else {
      // in double: an fp32 1 - powf(beta2, t) is 1e-4 off at t = 1
      c->step_size = lr / (1.0 - pow(b1, step));
      c->c1 = 1.0 / sqrt(1.0 - pow(b2, step));
      c->omb1 = 1.0 - b1;
      c->beta2 = b2;
      c->omb2 = 1.0 - b2;
      c->eps_or_nesterov = h[3];
    }
  }
}

// --------------------------------------------------------------------------------------------------------- step
// One element.  SGD in fp32 (three fused operations).  Adam in double from fp32 seeds: the chain g -> m, v -> sqrt -> quotient
// -> p is ~12 fp32 roundings, up to 6 ulp of the update where p is of the update's size, against a bound of 4; in double
// (about 20 FMAs per element, hidden under the memory traffic; sqrt and 1 / x are an fp32 result plus one Newton step) p is
// rounded once, and m and v once each on their way back to memory.
template <bool SGD>
__device__ __forceinline__ void update_one(float &p, float g, float &m, float &v, const OptimCoef &c, float gscale) {
  if (SGD) {
    const float mom = (float)c.c1;
    g = __builtin_fmaf((float)c.l2, p, g * gscale);
    m = __builtin_fmaf(mom, m, g);                                    // buf = momentum * buf + g (dampening 0)
    const float upd = c.eps_or_nesterov != 0.0 ? __builtin_fmaf(mom, m, g) : m;
    p = p - (float)c.step_size * upd;
  } else {
    const double gd = __builtin_fma(c.l2, (double)p, (double)g * (double)gscale);
    const double md = __builtin_fma(gd - (double)m, c.omb1, (double)m);
    const double vd = __builtin_fma(c.omb2 * gd, gd, (double)v * c.beta2);
    m = (float)md;
    v = (float)vd;
    const float s0 = sqrtf((float)vd);                                // below the fp32 range: 0, absolute error < 1e-19 beside eps
    const double s = s0 > 0.f ? __builtin_fma(vd - (double)s0 * (double)s0, (double)(0.5f / s0), (double)s0) : 0.0;
    const double denom = __builtin_fma(s, c.c1, c.eps_or_nesterov);
    const double r0 = (double)(1.0f / (float)denom);
    const double r = r0 * __builtin_fma(-denom, r0, 2.0);
    p = (float)__builtin_fma(-c.step_size * md, r, (double)p * c.decay_mul);
  }
}

template <bool SGD>
__device__ __forceinline__ void update_scalar(const OptimDesc &d, int64_t i, const OptimCoef &c, float gscale) {
  float p = d.p[i], m = d.m[i], v = 0.f;
  if (!SGD) v = d.v[i];
  update_one<SGD>(p, d.g[i], m, v, c, gscale);
  d.p[i] = p;
  d.m[i] = m;
  if (!SGD) d.v[i] = v;
}

// Registers: the 16 loads of an Adam thread are 64 VGPRs of data before the first use and the double arithmetic of an element
// needs register pairs, so the kernel does not fit the 64 VGPRs of eight waves per SIMD.  Compiled: Adam 115 VGPRs (bounded to
// four waves per SIMD, no scratch), SGD 76 VGPRs (six waves).  Measured at 43 M elements: 5.8 TB/s, 0.83 of m3_add_f32's rate.
template <bool SGD>
__global__ __launch_bounds__(256, 4) void optim_step_kernel(const OptimDesc *__restrict__ descs, int n_desc,
                                                         const float *__restrict__ state) {
  const OptimState *st = (const OptimState *)state;
  if (st->skip) return;                            // GradScaler's skipped step: p, m, v keep their bits
  const float gscale = st->gscale;
  const int b = blockIdx.x, t = threadIdx.x;
  const OptimDesc d = find_desc(descs, n_desc, b);
  const OptimCoef c = ((const OptimCoef *)(state + OPT_HEAD))[d.group];
  const int64_t base = (int64_t)(b - d.chunk_start) * OPT_CHUNK;
  const int64_t n4 = d.n & ~(int64_t)3;
  if (d.vec_ok && n4 > 0) {
    const int64_t left = n4 - base;
    const int valid = (int)(left < OPT_CHUNK ? left : OPT_CHUNK);
    float *pp = d.p + base, *pm = d.m + base, *pv = SGD ? nullptr : d.v + base;
    const float *pg = d.g + base;
    f32x4 P[OPT_PIECES], G[OPT_PIECES], M[OPT_PIECES], V[OPT_PIECES];
    int off[OPT_PIECES];
    // every load of every stream before the first use; a piece past the end re-reads the last whole float4 and is not stored
#pragma unroll
    for (int k = 0; k < OPT_PIECES; ++k) {
      const int e = (k * 256 + t) * 4;
      off[k] = e < valid ? e : valid - 4;
    }
#pragma unroll
    for (int k = 0; k < OPT_PIECES; ++k) G[k] = *(const f32x4 *)(pg + off[k]);
#pragma unroll
    for (int k = 0; k < OPT_PIECES; ++k) P[k] = *(const f32x4 *)(pp + off[k]);
#pragma unroll
    for (int k = 0; k < OPT_PIECES; ++k) M[k] = *(const f32x4 *)(pm + off[k]);
    if (!SGD) {
#pragma unroll
      for (int k = 0; k < OPT_PIECES; ++k) V[k] = *(const f32x4 *)(pv + off[k]);
    }
#pragma unroll
    for (int k = 0; k < OPT_PIECES; ++k) {
      f32x4 p = P[k], m = M[k], v = SGD ? f32x4{0.f, 0.f, 0.f, 0.f} : V[k];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = p[j], mj = m[j], vj = v[j];
        update_one<SGD>(pj, G[k][j], mj, vj, c, gscale);
        p[j] = pj; m[j] = mj; v[j] = vj;
      }
      if ((k * 256 + t) * 4 < valid) {
        *(f32x4 *)(pp + off[k]) = p;
        *(f32x4 *)(pm + off[k]) = m;
        if (!SGD) *(f32x4 *)(pv + off[k]) = v;
      }
    }
    const int64_t i = n4 + t;                                         // the up to 3 elements behind the last whole float4
    if (base + OPT_CHUNK >= d.n && i < d.n) update_scalar<SGD>(d, i, c, gscale);
  } else {
#pragma unroll 4
    for (int k = 0; k < OPT_PIECES * 4; ++k) {
      const int64_t i = base + k * 256 + t;
      if (i < d.n) update_scalar<SGD>(d, i, c, gscale);
    }
  }
}

}  // namespace m3

using namespace m3;

extern "C" int m3_optim_state_elems(int n_groups) { return n_groups < 1 ? 0 : OPT_HEAD + n_groups * (int)(sizeof(OptimCoef) / 4); }

static int optim_args_ok(const m3_optim_desc *descs, int n_desc, int total_chunks, const float *state, int kind, const char *who) {
  static_assert(sizeof(m3_optim_desc) == sizeof(OptimDesc), "descriptor layout");
  static_assert(sizeof(OptimState) == OPT_HEAD * 4 && sizeof(OptimCoef) == 64, "state layout");
  M3_REQUIRE(descs && n_desc >= 1 && total_chunks >= 1 && state, "%s: bad args", who);
  M3_REQUIRE(kind == M3_OPTIM_ADAMW || kind == M3_OPTIM_ADAM || kind == M3_OPTIM_SGD, "%s: bad kind %d", who, kind);
  return 0;
}

extern "C" int m3_optim_prepare(const m3_optim_desc *descs_dev, int n_desc, int total_chunks, const float *hyper, int n_groups,
                                int kind, const float *grad_scale, const float *found_inf_in, float max_norm, int want_norm,
                                float *partials, float *state, void *stream) {
  if (int rc = optim_args_ok(descs_dev, n_desc, total_chunks, state, kind, "m3_optim_prepare")) return rc;
  M3_REQUIRE(hyper && n_groups >= 1, "m3_optim_prepare: bad hyper-parameter table");
  M3_REQUIRE(!want_norm || partials, "m3_optim_prepare: want_norm needs the partials buffer (2 * total_chunks floats)");
  M3_REQUIRE(want_norm || !(max_norm > 0.f), "m3_optim_prepare: max_norm > 0 needs want_norm");
  hipStream_t s = (hipStream_t)stream;
  if (want_norm) {
    hipLaunchKernelGGL(optim_norm_kernel, dim3(total_chunks), dim3(256), 0, s, (const OptimDesc *)descs_dev, n_desc,
                       total_chunks, partials);
    if (int rc = check_launch("m3_optim_prepare (norm)")) return rc;
  }
  hipLaunchKernelGGL(optim_finalize_kernel, dim3(1), dim3(256), 0, s, partials, want_norm ? total_chunks : 0, hyper, n_groups,
                     kind, grad_scale, found_inf_in, max_norm, state);
  return check_launch("m3_optim_prepare (finalize)");
}

extern "C" int m3_optim_step(const m3_optim_desc *descs_dev, int n_desc, int total_chunks, const float *hyper,
                             const float *state, int kind, void *stream) {
  if (int rc = optim_args_ok(descs_dev, n_desc, total_chunks, state, kind, "m3_optim_step")) return rc;
  (void)hyper;                                     // the step reads the coefficients m3_optim_prepare derived into `state`
  hipStream_t s = (hipStream_t)stream;
  const OptimDesc *d = (const OptimDesc *)descs_dev;
  if (kind == M3_OPTIM_SGD) hipLaunchKernelGGL(optim_step_kernel<true>, dim3(total_chunks), dim3(256), 0, s, d, n_desc, state);
  else hipLaunchKernelGGL(optim_step_kernel<false>, dim3(total_chunks), dim3(256), 0, s, d, n_desc, state);
  return check_launch("m3_optim_step");
}
