// Routing statistics of one MoE block for gfx950, computed on the device inside the pass: what the reference's Block
// leaves in `last_moe_analysis` after seven .item() host reads (models/moe/ckpt/vision_transformer_moe.py:461-478,
// 540-562) - gate entropy, top-1 probability, the expert load histogram, the clean-logit spread, the MoE output / input
// norm ratio and the load CV - written as ONE small record in device memory that the host copies only when asked.
//
// Stage 1 follows the row-kernel idiom of combine.hip: one wave owns one token row at a time (rows are dealt to the waves of a
// fixed grid in a fixed order), lane e holds expert e of the row's gates / clean logits, the row of h and the k rows of y
// are read as 16-byte lane vectors that are all issued before the first use, everything accumulates in fp32, and every
// workgroup leaves one row of partials [nblk][5 + E] in the caller's workspace.  Stage 2 (one workgroup) adds the partials
// in block order and finishes the quotients, so two runs on the same inputs give the same bits.  No atomics.
#include "common.h"

namespace m3 {

constexpr int ST_THREADS = 256;        // 4 waves per workgroup
constexpr int ST_WAVES = ST_THREADS / 64;
constexpr int ST_MAX_BLOCKS = 512;     // two workgroups per CU: enough rows in flight for HBM, few enough partials for one workgroup
constexpr int ST_FIN_THREADS = 1024;
constexpr int ST_NF = 5;               // float partials: entropy, top-1, sum of row stds, |m|^2, |h|^2 - then E counts

static inline int stats_blocks(int64_t T) {
  const int64_t b = (T + ST_WAVES - 1) / ST_WAVES;
  return (int)(b < 1 ? 1 : (b > ST_MAX_BLOCKS ? ST_MAX_BLOCKS : b));
}

// KT: top-k as a template constant (1, 2, 4, 8; 0 = run-time k), as in combine_fwd_kernel: unrolled, the k row loads of a
// 16-byte column are in flight together.
template <typename T, int KT>
__global__ __launch_bounds__(ST_THREADS) void moe_stats_kernel(const float *__restrict__ score, const float *__restrict__ clean,
                                                               const float *__restrict__ gates, const T *__restrict__ h,
                                                               int64_t ldh, const T *__restrict__ y, int64_t ldy,
                                                               int64_t T_, int E, int k_rt, int D, float *__restrict__ ws) {
  constexpr int VE = 16 / (int)sizeof(T);               // one 16-byte lane vector of a row, as floats
  const int k = KT ? KT : k_rt;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const bool valid = lane < E;
  const int ec = valid ? lane : E - 1;                   // lanes past E re-read the last expert and contribute nothing
  const int nch = (D + 64 * VE - 1) / (64 * VE);
  float ent = 0.f, top1 = 0.f, stds = 0.f, msq = 0.f, hsq = 0.f;
  int cnt = 0;
  for (int64_t t = (int64_t)blockIdx.x * ST_WAVES + wave; t < T_; t += (int64_t)gridDim.x * ST_WAVES) {
    const float p = gates[t * E + ec];
    const float c = clean[t * E + ec];
    const float *sc = score + t * k;
    for (int ch = 0; ch < nch; ++ch) {
      const int col0 = lane * VE + ch * 64 * VE;
      const bool on = col0 < D;
      const int col = on ? col0 : 0;                     // unconditional loads: lanes past D re-read column 0
      float hv[VE], m[VE];
      Pack<T, VE>::load(h + t * ldh + col, hv);
      if constexpr (KT > 0) {
        float yv[KT][VE], sv[KT];
#pragma unroll
        for (int j = 0; j < KT; ++j) { Pack<T, VE>::load(y + (t * KT + j) * ldy + col, yv[j]); sv[j] = sc[j]; }
#pragma unroll
        for (int i = 0; i < VE; ++i) m[i] = 0.f;
#pragma unroll
        for (int j = 0; j < KT; ++j)                     // j = 0, 1, ...: the order of combine_fwd_kernel
#pragma unroll
          for (int i = 0; i < VE; ++i) m[i] = __builtin_fmaf(sv[j], yv[j][i], m[i]);
      } else {
#pragma unroll
        for (int i = 0; i < VE; ++i) m[i] = 0.f;
        for (int j = 0; j < k; ++j) {
          float yv[VE];
          Pack<T, VE>::load(y + (t * k + j) * ldy + col, yv);
          const float s = sc[j];
#pragma unroll
          for (int i = 0; i < VE; ++i) m[i] = __builtin_fmaf(s, yv[i], m[i]);
        }
      }
      if (on) {
#pragma unroll
        for (int i = 0; i < VE; ++i) { msq = __builtin_fmaf(m[i], m[i], msq); hsq = __builtin_fmaf(hv[i], hv[i], hsq); }
      }
    }
    // gate side: lane e owns expert e
    const float pv = valid ? p : 0.f;
    ent += valid ? -(p * logf(fmaxf(p, 1e-12f))) : 0.f;
    top1 += wave_max(pv);
    cnt += (valid && p > 0.f) ? 1 : 0;
    const float mu = wave_sum(valid ? c : 0.f) / (float)E;
    const float dl = valid ? c - mu : 0.f;
    stds += sqrtf(wave_sum(dl * dl) / (float)E);
  }
  __shared__ float s_f[ST_WAVES][ST_NF];
  __shared__ int s_c[ST_WAVES][64];
  ent = wave_sum(ent); msq = wave_sum(msq); hsq = wave_sum(hsq);
  if (lane == 0) { s_f[wave][0] = ent; s_f[wave][1] = top1; s_f[wave][2] = stds; s_f[wave][3] = msq; s_f[wave][4] = hsq; }
  s_c[wave][lane] = cnt;
  __syncthreads();
  const int S = ST_NF + E;
  float *out = ws + (int64_t)blockIdx.x * S;
  const int i = threadIdx.x;
  if (i < ST_NF) {
    float a = s_f[0][i];
#pragma unroll
    for (int w = 1; w < ST_WAVES; ++w) a += s_f[w][i];
    out[i] = a;
  } else if (i < S) {
    int a = 0;
#pragma unroll
    for (int w = 0; w < ST_WAVES; ++w) a += s_c[w][i - ST_NF];
    ((int32_t *)out)[i] = a;
  }
}

// Stage 2: the partials in block order (wave w takes blocks w, w + 16, ... - all of its at most 32 rows are loaded before the
// first add - and the 16 wave sums are then added 0, 1, ...), the quotients, and expert_load_cv = var_pop(load) /
// (mean(load)^2 + 1e-10) from the balance loss's own load vector (vision_transformer_moe.py:546-550; one wave, lane e holds
// load[e]) - the host never reads `load`.  A row of partials is 5 floats, then E counts: lane l adds word l (a float below
// ST_NF, else a count) and word 64 + l (a count).
__global__ __launch_bounds__(ST_FIN_THREADS) void moe_stats_finish_kernel(const float *__restrict__ ws, int nblk, int E,
                                                                          int64_t T_, const float *__restrict__ load_f32,
                                                                          const int64_t *__restrict__ load_i64,
                                                                          float *__restrict__ rec) {
  constexpr int NW = ST_FIN_THREADS / 64;
  constexpr int NR = ST_MAX_BLOCKS / NW;                 // rows of partials per wave
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int S = ST_NF + E;
  const uint32_t *wsu = (const uint32_t *)ws;
  __shared__ uint32_t s_w[NW][128];
  __shared__ float s_tot[ST_NF + 1];
  const int c0 = lane < S ? lane : S - 1, c1 = lane + 64 < S ? lane + 64 : S - 1;
  uint32_t w0[NR], w1[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) {                         // unconditional loads: rows past nblk re-read row 0
    const int b = wave + i * NW;
    const uint32_t *row = wsu + (int64_t)(b < nblk ? b : 0) * S;
    w0[i] = row[c0];
    w1[i] = row[c1];
  }
  float f = 0.f;
  int n0 = 0, n1 = 0;
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    if (wave + i * NW < nblk) {
      f += __uint_as_float(w0[i]);
      n0 += (int)w0[i];
      n1 += (int)w1[i];
    }
  }
  s_w[wave][lane] = lane < ST_NF ? __float_as_uint(f) : (uint32_t)n0;
  s_w[wave][64 + lane] = (uint32_t)n1;
  // the load CV, on wave 0 while the others finish
  float cv = 0.f;
  if (wave == 0 && E > 1) {
    const int ec = lane < E ? lane : E - 1;
    const float raw = load_f32 ? load_f32[ec] : (float)load_i64[ec];
    const float v = lane < E ? raw : 0.f;
    const float mean = wave_sum(v) / (float)E;
    const float d = lane < E ? v - mean : 0.f;
    cv = (wave_sum(d * d) / (float)E) / (mean * mean + 1e-10f);
  }
  __syncthreads();
  int32_t *reci = (int32_t *)rec;
  const int i = threadIdx.x;
  if (i < ST_NF) {
    float a = __uint_as_float(s_w[0][i]);
#pragma unroll
    for (int w = 1; w < NW; ++w) a += __uint_as_float(s_w[w][i]);
    s_tot[i] = a;
  } else if (i < S) {
    int a = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) a += (int)s_w[w][i];
    reci[M3_MOE_STATS_HIST + i - ST_NF] = a;
  }
  __syncthreads();
  if (i == 0) {
    rec[M3_MOE_STATS_ENTROPY_SUM] = s_tot[0];
    rec[M3_MOE_STATS_TOP1_SUM] = s_tot[1];
    rec[M3_MOE_STATS_CLEAN_STD] = T_ > 0 ? s_tot[2] / (float)T_ : 0.f;
    rec[M3_MOE_STATS_NORM_RATIO] = sqrtf(s_tot[3]) / (sqrtf(s_tot[4]) + 1e-12f);
    rec[M3_MOE_STATS_LOAD_CV] = cv;
    rec[M3_MOE_STATS_M_SUMSQ] = s_tot[3];
    rec[M3_MOE_STATS_H_SUMSQ] = s_tot[4];
    reci[M3_MOE_STATS_TOKENS] = (int32_t)T_;
  }
}

}  // namespace m3

using namespace m3;

extern "C" int64_t m3_moe_stats_ws_elems(int64_t T, int E) {
  if (T < 0 || E < 1 || E > 64) return 0;
  return (int64_t)stats_blocks(T) * (ST_NF + E);
}

extern "C" int m3_moe_stats(const float *score, const float *clean, const float *gates, const void *h, int64_t ldh,
                            const void *y, int64_t ldy, int dtype, const float *load_f32, const int64_t *load_i64,
                            int64_t T, int E, int k, int D, float *ws, void *record, void *stream) {
  M3_REQUIRE(score && clean && gates && h && y && ws && record, "m3_moe_stats: null operand");
  M3_REQUIRE((load_f32 != nullptr) != (load_i64 != nullptr), "m3_moe_stats: exactly one of load_f32 / load_i64");
  M3_REQUIRE(dtype_ok(dtype), "m3_moe_stats: bad dtype");
  M3_REQUIRE(E >= 1 && E <= 64 && k >= 1 && k <= E, "m3_moe_stats: E=%d outside [1,64] or k=%d outside [1,E]", E, k);
  M3_REQUIRE(T >= 0 && T < ((int64_t)1 << 31), "m3_moe_stats: T outside [0, 2^31)");
  const int es = dtype_size(dtype);
  M3_REQUIRE(D > 0 && (D * es) % 16 == 0 && ldh >= D && ldy >= D && (ldh * es) % 16 == 0 && (ldy * es) % 16 == 0 &&
                 ((uintptr_t)h % 16) == 0 && ((uintptr_t)y % 16) == 0,
             "m3_moe_stats: rows of h / y must be 16-byte multiples at 16-byte aligned addresses (D=%d)", D);
  hipStream_t s = (hipStream_t)stream;
  const int nblk = stats_blocks(T);
  by_dtype(dtype, [&](auto tt) {
    typedef typename decltype(tt)::type TT;
    auto go = [&](auto kt) {
      hipLaunchKernelGGL((moe_stats_kernel<TT, decltype(kt)::value>), dim3(nblk), dim3(ST_THREADS), 0, s, score, clean, gates,
                         (const TT *)h, ldh, (const TT *)y, ldy, T, E, k, D, ws);
    };
    if (!by_int<4, 2, 1, 8>(k, go)) go(IntTag<0>{});
  });
  int rc = check_launch("m3_moe_stats");
  if (rc != M3_OK) return rc;
  hipLaunchKernelGGL(moe_stats_finish_kernel, dim3(1), dim3(ST_FIN_THREADS), 0, s, (const float *)ws, nblk, E, T, load_f32,
                     load_i64, (float *)record);
  return check_launch("m3_moe_stats (finish)");
}
