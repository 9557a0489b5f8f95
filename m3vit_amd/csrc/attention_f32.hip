// Exact-fp32 attention forward / backward (any N, head dim 32 or 64).  Operands, softmax statistics, accumulators and LSE
// are fp32; every product is the exact 16x16x4 f32 MFMA (Mma<float>: a fragment is an f32x4 over 16 contraction elements).
// MFMA operand plan (16x16 tiles; "key on the lane" so that no accumulator ever has to move between lanes, cf.
// cdna_hip_programming.md App. B):
//   fwd : S^T[key][q] = K Q^T     (A = K rows from LDS, B = Q rows held in registers)
//         O^T[d][q]  += V^T P^T   (A = V^T from a transposed LDS image, B = the lane's own exp'd S^T values - C layout ==
//                                  B-operand layout)
//   bwd : one workgroup per (image, head, key block), each wave owns 64 keys and keeps dK^T / dV^T for them in registers
//         while sweeping 32-row query blocks: S[q][key] = Q K^T, dP = dO V^T (B = K / V fragments resident in registers);
//         dV^T += dO^T P, dK^T += Q^T dS (A from transposed LDS images of dO / Q, B = own registers); dS goes through LDS
//         once for dQ^T[d][q] = K^T dS^T.
#include "attention_dev.h"

namespace m3 {

typedef Mma<float> MM;
constexpr int AT_THREADS = 256;
constexpr int AT_KT = 64;       // keys per LDS tile (fwd)
constexpr int AT_QB = 64;       // query rows per workgroup (fwd): 4 waves x 16
constexpr int AT_KC = 16;       // contraction elements per fragment: 4 consecutive ones per lane group lg, at 4 * lg

template <int DH>
__global__ __launch_bounds__(AT_THREADS, 2) void attention_fwd_f32_kernel(const float *__restrict__ qkv, int B, int N, int heads,
                                                                           float *__restrict__ o, float *__restrict__ lse, float scale) {
  constexpr int NCH = DH / AT_KC, NDT = DH / 16;   // d chunks of the contraction, d tiles of the output
  constexpr int KSTR = DH * 4 + 16;         // bytes, sK row stride
  constexpr int VSTR = AT_KT * 4 + 16;      // bytes, sVt row stride
  constexpr int CPRK = DH * 4 / 16;         // 16-byte chunks (4 floats) per K/V row

  __shared__ __attribute__((aligned(16))) char sK[AT_KT * KSTR];
  __shared__ __attribute__((aligned(16))) char sVt[DH * VSTR];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  // XCD-aware order: the query blocks of one (image, head) and the neighbouring heads of the same
  // image (which share 128-byte lines of the packed qkv rows) get consecutive logical ids -> one XCD.
  const int nqb = gridDim.x;
  const int log_id = xcd_remap(blockIdx.x + nqb * blockIdx.y, nqb * gridDim.y);
  const int qb = log_id % nqb;
  const int bh = log_id / nqb, b = bh / heads, h = bh - b * heads;
  const int C = heads * DH;
  const int64_t ld = 3 * (int64_t)C;
  const float *qbase = qkv + (int64_t)b * N * ld + h * DH;
  const float *kbase = qbase + C, *vbase = qbase + 2 * C;

  const int q0 = qb * AT_QB + wave * 16;
  const int qrow = q0 + li;
  f32x4 qf[NCH];
#pragma unroll
  for (int ch = 0; ch < NCH; ++ch) {
    if (qrow < N) qf[ch] = *(const f32x4 *)(qbase + (int64_t)qrow * ld + ch * AT_KC + 4 * lg);
    else qf[ch] = MM::zero();
  }

  f32x4 oacc[NDT];
#pragma unroll
  for (int i = 0; i < NDT; ++i) oacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;

  for (int key0 = 0; key0 < N; key0 += AT_KT) {
    __syncthreads();
    // ---- stage K rows and V^T
    for (int q = tid; q < AT_KT * CPRK; q += AT_THREADS) {
      const int row = q / CPRK, c = q - row * CPRK;
      const int key = key0 + row;
      u32x4 kv = u32x4{0u, 0u, 0u, 0u}, vv = u32x4{0u, 0u, 0u, 0u};
      if (key < N) {
        kv = *(const u32x4 *)((const char *)(kbase + (int64_t)key * ld) + c * 16);
        vv = *(const u32x4 *)((const char *)(vbase + (int64_t)key * ld) + c * 16);
      }
      *(u32x4 *)(sK + row * KSTR + c * 16) = kv;
      const float *ve = (const float *)&vv;
#pragma unroll
      for (int j = 0; j < 4; ++j) *(float *)(sVt + (c * 4 + j) * VSTR + row * 4) = ve[j];
    }
    __syncthreads();

    // ---- S^T tiles: [key = 16*kt + 4*lg + r][q = li]
    f32x4 st[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      st[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        const f32x4 kf = *(const f32x4 *)(sK + (kt * 16 + li) * KSTR + (ch * AT_KC + 4 * lg) * 4);
        st[kt] = MM::mma(kf, qf[ch], st[kt]);
      }
    }
    float mt = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int key = key0 + kt * 16 + 4 * lg + r;
        const float s = (key < N) ? st[kt][r] * scale : -INFINITY;
        st[kt][r] = s;
        mt = fmaxf(mt, s);
      }
    mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
    mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
    const float m_new = fmaxf(m_run, mt);
    const float alpha = __expf(m_run - m_new);
    float psum = 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = __expf(st[kt][r] - m_new);
        st[kt][r] = p;
        psum += p;
      }
    l_run = l_run * alpha + psum;
    m_run = m_new;
#pragma unroll
    for (int i = 0; i < NDT; ++i) oacc[i] *= alpha;

    // ---- O^T += V^T P^T : one 16-key S^T tile is one B fragment
#pragma unroll
    for (int cc = 0; cc < AT_KT / AT_KC; ++cc) {
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        const f32x4 vf = *(const f32x4 *)((const float *)(sVt + (dt * 16 + li) * VSTR) + cc * AT_KC + 4 * lg);
        oacc[dt] = MM::mma(vf, st[cc], oacc[dt]);
      }
    }
  }

  float l_tot = l_run + __shfl_xor(l_run, 16, 64);
  l_tot += __shfl_xor(l_tot, 32, 64);
  if (qrow < N) {
    const float inv = 1.0f / l_tot;
    float *orow = o + ((int64_t)b * N + qrow) * C + h * DH;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) *(f32x4 *)(orow + dt * 16 + 4 * lg) = oacc[dt] * inv;
    if (lg == 0) lse[((int64_t)b * heads + h) * N + qrow] = m_run + __logf(l_tot);
  }
}

// ------------------------------------------------------------------------ backward
constexpr int AB_QB = 32;                       // query rows per step: two 16-query fragments
// LDS images of the backward, row strides in bytes
template <int DH> struct AbLds {
  static constexpr int RSTR = DH * 4 + 16;          // row-major Q / dO images
  static constexpr int TSTR = AB_QB * 4 + 16;       // transposed Q^T / dO^T images
  static constexpr int SSTR = ATTN_KEYS * 4 + 16;   // K^T and dS images (keys contiguous)
  static constexpr size_t BYTES = (size_t)DH * SSTR + (size_t)AB_QB * SSTR + 2 * (size_t)AB_QB * RSTR + 2 * (size_t)DH * TSTR +
                                  2 * AB_QB * sizeof(float);
};

template <int DH>
__global__ __launch_bounds__(AT_THREADS, 1) void attention_bwd_f32_kernel(const float *__restrict__ qkv, const float *__restrict__ o,
                                                                           const float *__restrict__ d_o, const float *__restrict__ lse,
                                                                           int B, int N, int heads, float *__restrict__ dqkv,
                                                                           float *__restrict__ dq_ws, float scale) {
  constexpr int NCH = DH / AT_KC, NDT = DH / 16;
  constexpr int RSTR = AbLds<DH>::RSTR, TSTR = AbLds<DH>::TSTR, SSTR = AbLds<DH>::SSTR;
  constexpr int CPR = DH * 4 / 16;                // 16-byte chunks (4 floats) per row

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char *sKt = smem;                               // [DH][SSTR]
  char *sdS = sKt + DH * SSTR;                    // [AB_QB][SSTR]
  char *sQ = sdS + AB_QB * SSTR;                  // [AB_QB][RSTR]
  char *sdO = sQ + AB_QB * RSTR;
  char *sQt = sdO + AB_QB * RSTR;                 // [DH][TSTR]
  char *sdOt = sQt + DH * TSTR;
  float *sLse = (float *)(sdOt + DH * TSTR);      // [AB_QB]
  float *sDelta = sLse + AB_QB;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  // one workgroup per (image, head, 256-key block); the key blocks of one (image, head) read the same Q / dO
  // rows and neighbouring heads share lines: consecutive logical ids -> one XCD
  const int nkb = (N + ATTN_KEYS - 1) / ATTN_KEYS;
  const int wid = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = wid / nkb, kbi = wid - bh * nkb, b = bh / heads, h = bh - b * heads;
  const int C = heads * DH;
  const int64_t ld = 3 * (int64_t)C;
  const float *qbase = qkv + (int64_t)b * N * ld + h * DH;
  const float *kbase = qbase + C, *vbase = qbase + 2 * C;
  const float *obase = o + (int64_t)b * N * C + h * DH;
  const float *dobase = d_o + (int64_t)b * N * C + h * DH;
  float *dqbase = dqkv + (int64_t)b * N * ld + h * DH;
  const float *lbase = lse + ((int64_t)b * heads + h) * N;
  const int kw0 = wave * 64;

  // Sequences longer than ATTN_KEYS keys: each key block has its own workgroup.  dK/dV of a key block are
  // complete after its sweep over the queries; its dQ contribution goes to an fp32 slab
  // dq_ws[key block][image, head][N][DH], summed in key-block order by attention_dq_reduce_kernel (deterministic).
  const int64_t nbh = gridDim.x / nkb;
  float *dqw = dq_ws ? dq_ws + ((int64_t)kbi * nbh + bh) * N * DH : nullptr;
  const int kb0 = kbi * ATTN_KEYS;
  __syncthreads();
  // ---- K^T image (all keys) + this wave's K / V fragments
  for (int q = tid; q < ATTN_KEYS * CPR; q += AT_THREADS) {
    const int row = q / CPR, c = q - row * CPR;
    u32x4 kv = u32x4{0u, 0u, 0u, 0u};
    if (kb0 + row < N) kv = *(const u32x4 *)((const char *)(kbase + (int64_t)(kb0 + row) * ld) + c * 16);
    const float *ke = (const float *)&kv;
#pragma unroll
    for (int j = 0; j < 4; ++j) *(float *)(sKt + (c * 4 + j) * SSTR + row * 4) = ke[j];
  }
  f32x4 kf[4][NCH], vf[4][NCH];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
    const int key = kb0 + kw0 + kt * 16 + li;
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      if (key < N) {
        kf[kt][ch] = *(const f32x4 *)(kbase + (int64_t)key * ld + ch * AT_KC + 4 * lg);
        vf[kt][ch] = *(const f32x4 *)(vbase + (int64_t)key * ld + ch * AT_KC + 4 * lg);
      } else {
        kf[kt][ch] = MM::zero();
        vf[kt][ch] = MM::zero();
      }
    }
  }
  f32x4 dkt[NDT][4], dvt[NDT][4];
#pragma unroll
  for (int a = 0; a < NDT; ++a)
#pragma unroll
    for (int c = 0; c < 4; ++c) { dkt[a][c] = f32x4{0.f, 0.f, 0.f, 0.f}; dvt[a][c] = f32x4{0.f, 0.f, 0.f, 0.f}; }

  const int nkeys = (N - kb0 < ATTN_KEYS) ? N - kb0 : ATTN_KEYS;
  const int nkc = (nkeys + AT_KC - 1) / AT_KC;   // key chunks that matter for dQ

  for (int qs = 0; qs < N; qs += AB_QB) {
    __syncthreads();
    // ---- stage Q, dO (row-major + transposed), lse, delta
    for (int q = tid; q < AB_QB * CPR; q += AT_THREADS) {
      const int row = q / CPR, c = q - row * CPR;
      const int qr = qs + row;
      u32x4 qv = u32x4{0u, 0u, 0u, 0u}, dv = u32x4{0u, 0u, 0u, 0u};
      if (qr < N) {
        qv = *(const u32x4 *)((const char *)(qbase + (int64_t)qr * ld) + c * 16);
        dv = *(const u32x4 *)((const char *)(dobase + (int64_t)qr * C) + c * 16);
      }
      *(u32x4 *)(sQ + row * RSTR + c * 16) = qv;
      *(u32x4 *)(sdO + row * RSTR + c * 16) = dv;
      const float *qe = (const float *)&qv, *de = (const float *)&dv;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        *(float *)(sQt + (c * 4 + j) * TSTR + row * 4) = qe[j];
        *(float *)(sdOt + (c * 4 + j) * TSTR + row * 4) = de[j];
      }
    }
    {
      // delta[row] = sum_d dO*O ; 8 threads per row
      const int row = tid >> 3, part = tid & 7;
      const int qr = qs + row;
      float s = 0.f;
      if (qr < N) {
        constexpr int PER = DH / 8;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
          const int d = part * PER + j;
          s += dobase[(int64_t)qr * C + d] * obase[(int64_t)qr * C + d];
        }
      }
      s += __shfl_xor(s, 1, 64);
      s += __shfl_xor(s, 2, 64);
      s += __shfl_xor(s, 4, 64);
      if (part == 0) {
        sDelta[row] = s;
        sLse[row] = (qr < N) ? lbase[qr] : 0.f;
      }
    }
    __syncthreads();

    // ---- S, dP -> P, dS for this wave's 64 keys
    f32x4 pt[2][4], dst[2][4];
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      f32x4 qfr[NCH], dof[NCH];
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        qfr[ch] = *(const f32x4 *)(sQ + (qt * 16 + li) * RSTR + (ch * AT_KC + 4 * lg) * 4);
        dof[ch] = *(const f32x4 *)(sdO + (qt * 16 + li) * RSTR + (ch * AT_KC + 4 * lg) * 4);
      }
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
        f32x4 s = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int ch = 0; ch < NCH; ++ch) {
          s = MM::mma(qfr[ch], kf[kt][ch], s);      // D[q = 4*lg + r][key = li]
          dp = MM::mma(dof[ch], vf[kt][ch], dp);
        }
        const int key = kb0 + kw0 + kt * 16 + li;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int ql = qt * 16 + 4 * lg + r;
          const bool ok = (key < N) && (qs + ql < N);
          const float p = ok ? __expf(s[r] * scale - sLse[ql]) : 0.f;
          pt[qt][kt][r] = p;
          dst[qt][kt][r] = p * (dp[r] - sDelta[ql]) * scale;
        }
      }
    }
    // ---- dV^T += dO^T P ; dK^T += Q^T dS   (contraction over the 32 queries: the P / dS tile of each 16-query
    // half is one B fragment)
#pragma unroll
    for (int qc = 0; qc < 2; ++qc) {
      f32x4 aq[NDT], ado[NDT];
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        aq[dt] = *(const f32x4 *)((const float *)(sQt + (dt * 16 + li) * TSTR) + qc * AT_KC + 4 * lg);
        ado[dt] = *(const f32x4 *)((const float *)(sdOt + (dt * 16 + li) * TSTR) + qc * AT_KC + 4 * lg);
      }
#pragma unroll
      for (int kt = 0; kt < 4; ++kt) {
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
          dvt[dt][kt] = MM::mma(ado[dt], pt[qc][kt], dvt[dt][kt]);
          dkt[dt][kt] = MM::mma(aq[dt], dst[qc][kt], dkt[dt][kt]);
        }
      }
    }
    // ---- dS -> LDS [q][key]
#pragma unroll
    for (int qt = 0; qt < 2; ++qt)
#pragma unroll
      for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          *(float *)(sdS + (qt * 16 + 4 * lg + r) * SSTR + (kw0 + kt * 16 + li) * 4) = dst[qt][kt][r];
    __syncthreads();
    // ---- dQ^T[d][q] = K^T dS^T : pieces (qt, dt) dealt to the waves
    for (int piece = wave; piece < 2 * NDT; piece += 4) {
      const int qt = piece / NDT, dt = piece - qt * NDT;
      f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
      for (int c = 0; c < nkc; ++c) {
        const f32x4 a = *(const f32x4 *)(sKt + (dt * 16 + li) * SSTR + (c * AT_KC + 4 * lg) * 4);
        const f32x4 bq = *(const f32x4 *)(sdS + (qt * 16 + li) * SSTR + (c * AT_KC + 4 * lg) * 4);
        acc = MM::mma(a, bq, acc);                   // D[d = 4*lg + r][q = li]
      }
      const int qr = qs + qt * 16 + li;
      if (qr < N) {
        if (dqw) *(f32x4 *)(dqw + (int64_t)qr * DH + dt * 16 + 4 * lg) = acc;
        else *(f32x4 *)(dqbase + (int64_t)qr * ld + dt * 16 + 4 * lg) = acc;
      }
    }
  }

  // ---- dK, dV rows of this wave's keys
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) {
    const int key = kb0 + kw0 + kt * 16 + li;
    if (key < N) {
#pragma unroll
      for (int dt = 0; dt < NDT; ++dt) {
        *(f32x4 *)(dqbase + C + (int64_t)key * ld + dt * 16 + 4 * lg) = dkt[dt][kt];
        *(f32x4 *)(dqbase + 2 * C + (int64_t)key * ld + dt * 16 + 4 * lg) = dvt[dt][kt];
      }
    }
  }
}

int launch_attention_fwd_f32(const void *qkv, int B, int N, int heads, int dh, void *o, float *lse, float scale, hipStream_t s) {
  const dim3 grid((N + AT_QB - 1) / AT_QB, B * heads), block(AT_THREADS);
  if (dh == 32)
    hipLaunchKernelGGL((attention_fwd_f32_kernel<32>), grid, block, 0, s, (const float *)qkv, B, N, heads, (float *)o, lse, scale);
  else
    hipLaunchKernelGGL((attention_fwd_f32_kernel<64>), grid, block, 0, s, (const float *)qkv, B, N, heads, (float *)o, lse, scale);
  return check_launch("m3_attention_fwd");
}

template <int DH>
static int launch_attn_bwd_f32(const void *qkv, const void *o, const void *d_o, const float *lse, int B, int N, int heads,
                               void *dqkv, float *dq_ws, float scale, hipStream_t s) {
  constexpr size_t lds = AbLds<DH>::BYTES;
  static bool attr_set = false;
  if (!attr_set) {
    if (lds > 64 * 1024)
      (void)hipFuncSetAttribute((const void *)attention_bwd_f32_kernel<DH>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_set = true;
  }
  hipLaunchKernelGGL((attention_bwd_f32_kernel<DH>), dim3(B * heads * attn_key_blocks(N)), dim3(AT_THREADS), lds, s,
                     (const float *)qkv, (const float *)o, (const float *)d_o, lse, B, N, heads, (float *)dqkv, dq_ws, scale);
  return check_launch("m3_attention_bwd");
}

int launch_attention_bwd_f32(const void *qkv, const void *o, const void *d_o, const float *lse, int B, int N, int heads, int dh,
                             void *dqkv, float *dq_ws, float scale, hipStream_t s) {
  if (dh == 32) return launch_attn_bwd_f32<32>(qkv, o, d_o, lse, B, N, heads, dqkv, dq_ws, scale, s);
  return launch_attn_bwd_f32<64>(qkv, o, d_o, lse, B, N, heads, dqkv, dq_ws, scale, s);
}

}  // namespace m3
