// The register-staged weight-gradient kernel (wgrad_tn_kernel) and its launcher; wgrad.hip describes the call.  Compiled as part of
// wgrad_tiles.hip.
// Both operands are row-major with the contraction index as the ROW, so fragments must
// be read transposed out of LDS:
//   f16: ds_read_b64_tr_b16 (4 rows x 16 cols per 16-lane group) on a [32][128]+pad
//        image, row stride 288 B -> the 8 rows one 32-lane half touches land on
//        8 disjoint 8-bank windows (conflict free);
//   f32: ds_read_b32 (each lane one element) on a 528 B stride image (conflict free).
// 128(n) x 128(k) output tile per 256-thread workgroup (2x2 waves of 64x64), 32 rows per
// barrier step, double-buffered register staging.  Rows are split `splits` ways;
// each split writes an fp32 slab, m3_wgrad_reduce adds the slabs in a fixed order
// (deterministic, unlike atomics).
#include "wgrad_dev.h"

namespace m3 {

template <typename T> struct WgLds;
// ROWS: contraction rows per barrier step.  (fp16 with 64 rows - 32 MFMAs per wave per barrier instead of 16 - was
// built in round 2: the second pair of staging registers spills, 256 VGPRs + 172 B scratch, and the step got 1-2 %
// slower.)
template <> struct WgLds<half_t> { static constexpr int STRIDE = 288; static constexpr int ROWS = 32; };
template <> struct WgLds<bf16_t> { static constexpr int STRIDE = 288; static constexpr int ROWS = 32; };
template <> struct WgLds<float> { static constexpr int STRIDE = 528; static constexpr int ROWS = 32; };

// fragment for 16 columns starting at byte column offset colb (col*sizeof(T)) of the
// LDS image `base`, contraction rows rb .. rb+KC-1
template <typename T>
__device__ __forceinline__ typename Mma<T>::frag read_tr_frag(const char *base, int rb, int col, int li, int lg);

template <>
__device__ __forceinline__ f16x8 read_tr_frag<half_t>(const char *base, int rb, int col, int li, int lg) {
  // lane li of group lg supplies the address of (row 4*lg + (li>>2) [+16], cols col + 4*(li&3))
  const char *p0 = base + (rb + 4 * lg + (li >> 2)) * WgLds<half_t>::STRIDE + (col + 4 * (li & 3)) * 2;
  const char *p1 = p0 + 16 * WgLds<half_t>::STRIDE;
  return wgrad_tr16_frag(p0, p1);
}

template <>
__device__ __forceinline__ bf16x8 read_tr_frag<bf16_t>(const char *base, int rb, int col, int li, int lg) {
  // the 16-bit transposed read does not look at the element format: same addressing as f16, bits re-labelled
  return __builtin_bit_cast(bf16x8, read_tr_frag<half_t>(base, rb, col, li, lg));
}

template <>
__device__ __forceinline__ f32x4 read_tr_frag<float>(const char *base, int rb, int col, int li, int lg) {
  const char *p = base + (rb + 4 * lg) * WgLds<float>::STRIDE + (col + li) * 4;
  f32x4 f;
  f[0] = *(const float *)(p);
  f[1] = *(const float *)(p + WgLds<float>::STRIDE);
  f[2] = *(const float *)(p + 2 * WgLds<float>::STRIDE);
  f[3] = *(const float *)(p + 3 * WgLds<float>::STRIDE);
  return f;
}

// Diagnostic build only (make CXXFLAGS+=-DM3_WGRAD_STAMPS, tools/wgrad_tn_stamps.py): lane 0 of wave 0 of the workgroups of
// output tile 0 (one per work unit or row part) records s_memtime at entry, after the prologue and four times per 32-row
// step of the steady-state loop - loads issued, MFMAs issued, LDS stores issued (the step's data has arrived), barrier
// passed.  No stamp executes in the shipped kernel.
#ifdef M3_WGRAD_STAMPS
constexpr int WTSTAMP_WGS = 128, WTSTAMP_N = 2 + 4 * 80;
__device__ unsigned long long g_wtn_stamps[WTSTAMP_WGS][WTSTAMP_N];
#define WT_STAMP(i)                                                                                                   \
  do {                                                                                                                \
    const int wg_ = blockIdx.y + gridDim.y * blockIdx.z;                                                              \
    if (threadIdx.x == 0 && blockIdx.x == 0 && wg_ < WTSTAMP_WGS && (i) < WTSTAMP_N)                                  \
      g_wtn_stamps[wg_][(i)] = __builtin_amdgcn_s_memtime();                                                          \
  } while (0)
#else
#define WT_STAMP(i) do { } while (0)
#endif

// One workgroup's work once it knows what is its own: output tile `tile` of group g over the 32-row steps s_begin .. s_begin +
// nst - 1 of the rows r0 .. r1 - 1, result to slab `slab_id` (or into dW: direct mode).  Shared by wgrad_tn_kernel and the
// batched wgrad_multi_kernel (wgrad_multi.hip).
template <typename T, bool GC, bool GA, bool SC>
__device__ __forceinline__ void wgrad_tile_loop(const WgradDev &p, int tile, int g, int64_t slab_id, int64_t r0, int64_t r1,
                                                int64_t s_begin, int nst) {
  typedef Mma<T> MM;
  typedef typename MM::frag frag;
  constexpr int ES = (int)sizeof(T);
  constexpr int EPC = 16 / ES;
  constexpr int STRIDE = WgLds<T>::STRIDE;
  constexpr int ROWS = WgLds<T>::ROWS;                      // contraction rows per step
  constexpr int CPR = WG_T * ES / 16;                       // 16-byte chunks per tile row
  constexpr int NLD = ROWS * CPR / WG_THREADS;           // chunks per thread per operand
  constexpr int RSTEP = WG_THREADS / CPR;                   // tile rows between a thread's chunks
  constexpr int OPB = ROWS * STRIDE;                     // bytes per operand image
  constexpr int KCH = ROWS / MM::KC;                     // fragment chunks per step

  extern __shared__ __attribute__((aligned(16))) char smem[];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int wr = wave >> 1, wc = wave & 1;

  const int tn = tile / p.tiles_k, tk = tile - tn * p.tiles_k;
  const int n0 = tn * WG_T, k0 = tk * WG_T;

  f32x4 acc[4][4];   // [ki][ni]: MFMA rows = k, cols = n
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};

  // staging assignment: chunk i of this thread is tile row (tid / CPR) + RSTEP*i, 16-byte column c.
  // Columns beyond N / K are clamped (they only feed outputs that are never stored); rows beyond the
  // end of the group are clamped for the load and ZEROED at the LDS store (they would otherwise add
  // into every output).  Loads are unconditional so hipcc's counted vmcnt waits stay exact.
  const int srow = tid / CPR, c = tid - srow * CPR;
  int ncol = n0 + c * EPC, kcol = k0 + c * EPC;
  if (ncol > p.N - EPC) ncol = p.N - EPC;
  if (kcol > p.K - EPC) kcol = p.K - EPC;
  const char *c_base = p.dC + (int64_t)ncol * ES;
  const char *a_base = p.A + (int64_t)kcol * ES;
  const int st_off = srow * STRIDE + c * 16;                // + i*RSTEP*STRIDE
  // Rows and row strides in 32 bits (M < 2^31 and strides below 4 GiB: the entry points check both), so that a row's byte
  // offset is ONE 32 x 32 -> 64-bit multiply-add onto the base.  As int64_t row * int64_t stride every address was three
  // quarter-rate multiplies + the add, four addresses per half step: half of the time between a barrier and the last load
  // request of a plain-row launch (profiles/expert_wgrad_units.txt).
  const uint32_t ldc = (uint32_t)p.lddc_b, lda = (uint32_t)p.lda_b;
  const uint32_t rfirst = (uint32_t)(r0 + s_begin * ROWS);            // row 0 of local step 0
  const uint32_t rbase = rfirst + (uint32_t)srow;                     // row of chunk 0 in local step 0
  const uint32_t rend = (uint32_t)r1;

  auto row_of = [&](int step, int i) -> uint32_t {          // clamped slot row (called with nst > 0 only: r1 > r0 >= 0)
    const uint32_t m = rbase + (uint32_t)(step * ROWS + i * RSTEP);
    return m < rend ? m : rend - 1;
  };
  // The gather table (GC / GA): what a gathered row needs - its source row, index already divided, and with SC its factor -
  // is loaded ONCE per row and workgroup and kept in LDS behind the operand images, in pieces of WG_TAB_ROWS rows (8 steps),
  // thread r owning row r of a piece, two slots: the entry of local row l is l mod 2 * WG_TAB_ROWS.  Rows past r1 clamp to
  // r1 - 1 (their data is zeroed at the LDS store).  (The 16 threads of a row each loaded the row's index and factor
  // themselves before: two index and two factor loads per thread and step in the queue of the data loads -
  // profiles/wgrad_steady_loop.txt.)  A piece is made in three stages:
  //   request (index -> ti), factor (c_row_scale[ti] -> tf), write (rows and factor -> LDS, published by the next barrier).
  // The prologue makes the pieces 0 and 1; the loop over whole pieces (four pairs of steps, unrolled: every stage at a fixed
  // place, no branch - behind a branch hipcc copies ti / tf where the paths join, and the copy of a register just loaded is a
  // wait for everything in flight) makes piece j + 2 while it computes piece j: request and factor at the START of the pairs
  // 0 and 1, in front of their data loads, so that waiting for them drains only loads the LDS stores have waited for
  // already; write in the middle of pair 3, behind the barrier after which nobody reads piece j any more.  When that loop
  // ends, at most 10 steps are left and their two pieces are in the table.
  constexpr int TMASK = 2 * WG_TAB_ROWS - 1;
  static_assert(WG_TAB_ROWS % ROWS == 0 && WG_TAB_ROWS / ROWS == 8, "a piece is four pairs of steps");
  uint32_t *tab_c = (uint32_t *)(smem + 2 * (2 * OPB));
  float *tab_f = (float *)(tab_c + 2 * WG_TAB_ROWS);
  uint32_t *tab_a = (uint32_t *)(tab_f + 2 * WG_TAB_ROWS);
  auto tab_request = [&](int piece, int32_t &xc, int32_t &xa) {
    uint32_t m = rfirst + (uint32_t)(piece * WG_TAB_ROWS + tid);
    m = m < rend ? m : rend - 1;
    if (GC) xc = p.c_row_idx[m];
    if (GA) xa = p.a_row_idx[m];
  };
  auto tab_factor = [&](int32_t xc, float &f) {
    if (SC) f = p.c_row_scale[xc];
  };
  auto tab_write_rows = [&](int piece, int32_t xc, int32_t xa) {
    const int e = (piece & 1) * WG_TAB_ROWS + tid;
    if (GC) tab_c[e] = (uint32_t)div_by(xc, p.c_row_div, p.c_row_sh);
    if (GA) tab_a[e] = (uint32_t)div_by(xa, p.a_row_div, p.a_row_sh);
  };
  auto tab_write_factor = [&](int piece, float f) {
    if (SC) tab_f[(piece & 1) * WG_TAB_ROWS + tid] = f;
  };
  // the source rows / the factors of this thread's chunks of `step` (whose piece is in the table)
  auto tab_rows = [&](int step, uint32_t(&nc)[NLD], uint32_t(&na)[NLD]) {
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const int e = (step * ROWS + srow + i * RSTEP) & TMASK;
      if (GC) nc[i] = tab_c[e];
      if (GA) na[i] = tab_a[e];
    }
  };
  auto tab_factors = [&](int step, float(&rs)[NLD]) {
#pragma unroll
    for (int i = 0; i < NLD; ++i)
      if (SC) rs[i] = tab_f[(step * ROWS + srow + i * RSTEP) & TMASK];
  };
  // Two forms of the load and of the LDS store, chosen at compile time by `whole`.
  // false_type: any step - rows clamped (row_of), one multiply-add per address, rows past the end zeroed at the store.
  // true_type: a WHOLE step (all 32 rows below r1: every step of a part but its last) that directly follows the step loaded
  // before - a plain operand's chunk addresses are the pointers pc / pa, bumped by the loop-invariant ROWS * ld after each
  // use (no clamp, no multiply: profiles/wgrad_steady_loop.txt), and the store writes the registers as they are.
  // A gathered operand's address is one multiply-add of its table row (nc / na) in both forms.
  typedef std::false_type any_step;
  typedef std::true_type whole_step;
  const char *pc[NLD], *pa[NLD];
  const uint64_t bump_c = (uint64_t)ROWS * ldc, bump_a = (uint64_t)ROWS * lda;
  auto point_at = [&](int step) {                           // pc / pa: the plain-row chunk addresses of `step`
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const uint32_t m = rbase + (uint32_t)(step * ROWS + i * RSTEP);
      pc[i] = c_base + (uint64_t)m * ldc;
      pa[i] = a_base + (uint64_t)m * lda;
    }
  };
  auto load_global = [&](auto whole, int step, const uint32_t(&nc)[NLD], const uint32_t(&na)[NLD], u32x4(&rc)[NLD],
                         u32x4(&ra)[NLD]) {
    constexpr bool W = decltype(whole)::value;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const char *cp, *ap;
      if constexpr (GC) cp = c_base + (uint64_t)nc[i] * ldc;
      else if constexpr (W) { cp = pc[i]; pc[i] += bump_c; }
      else cp = c_base + (uint64_t)row_of(step, i) * ldc;
      if constexpr (GA) ap = a_base + (uint64_t)na[i] * lda;
      else if constexpr (W) { ap = pa[i]; pa[i] += bump_a; }
      else ap = a_base + (uint64_t)row_of(step, i) * lda;
      rc[i] = *(const u32x4 *)cp;
      ra[i] = *(const u32x4 *)ap;
    }
  };
  auto store_lds = [&](auto whole, int buf, int step, const u32x4(&rc)[NLD], const u32x4(&ra)[NLD], const float(&rs)[NLD]) {
    constexpr bool W = decltype(whole)::value;
    char *base = smem + buf * (2 * OPB) + st_off;
#pragma unroll
    for (int i = 0; i < NLD; ++i) {
      const bool ok = W || rbase + (uint32_t)(step * ROWS + i * RSTEP) < rend;
      const u32x4 cv = SC ? scale_chunk<T>(rc[i], rs[i]) : rc[i];
      *(u32x4 *)(base + i * RSTEP * STRIDE) = ok ? cv : u32x4{0u, 0u, 0u, 0u};
      *(u32x4 *)(base + i * RSTEP * STRIDE + OPB) = ok ? ra[i] : u32x4{0u, 0u, 0u, 0u};
    }
  };
  // Bias gradient fused as one extra MFMA row: with an all-ones A operand the product is the column
  // sum of dC over the contraction rows.  Done once per n-tile (k-tile 0, waves wr == 0).
  const bool do_bias = (p.bias_ws || p.direct_db) && tk == 0 && wr == 0;
  f32x4 acc_b[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc_b[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  frag ones;
#pragma unroll
  for (int j = 0; j < MM::EPL; ++j) ones[j] = (T)1.0f;

  auto compute = [&](int buf) {
    const char *sC = smem + buf * (2 * OPB), *sA = sC + OPB;
#pragma unroll
    for (int kc = 0; kc < KCH; ++kc) {
      frag fk[4], fn[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        fk[i] = read_tr_frag<T>(sA, kc * MM::KC, wr * 64 + i * 16, li, lg);
        fn[i] = read_tr_frag<T>(sC, kc * MM::KC, wc * 64 + i * 16, li, lg);
      }
#pragma unroll
      for (int ki = 0; ki < 4; ++ki)
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc[ki][ni] = MM::mma(fk[ki], fn[ni], acc[ki][ni]);
      if (do_bias) {
#pragma unroll
        for (int ni = 0; ni < 4; ++ni) acc_b[ni] = MM::mma(ones, fn[ni], acc_b[ni]);
      }
    }
  };

  WT_STAMP(0);                                    // entry
  if (nst > 0) {
    // prefetch distance 2 for the data (two register sets); a gathered operand's rows come from the table one fetch ahead
    // (nc / na: read behind the loads of step s for step s + 1 - an LDS read, not in the queue of the data).  Steps past
    // the end re-load the last step (clamped) so that nothing in the steady-state loop is conditional but the table stages.
    const int last = nst - 1;
    auto cl = [&](int s_) { return s_ < last ? s_ : last; };
    u32x4 rc0[NLD], ra0[NLD], rc1[NLD], ra1[NLD];
    uint32_t nc[NLD] = {}, na[NLD] = {};
    float rs[NLD] = {};
    // (fp32, which spills as it is, with ONE gather: the rows of step ds are read in front of its loads - NLD = 4 rows kept
    // over a step cost it 16 more bytes of scratch; with both gathers it is the other way round)
    constexpr bool AHEAD = ES == 2 || (GC && GA);
    auto fetch = [&](auto whole, int ds, u32x4(&rc)[NLD], u32x4(&ra)[NLD]) {
      if constexpr (!AHEAD) tab_rows(ds, nc, na);
      load_global(whole, ds, nc, na, rc, ra);
      if constexpr (AHEAD) tab_rows(cl(ds + 1), nc, na);
    };
    auto store_step = [&](int buf, int step, const u32x4(&rc)[NLD], const u32x4(&ra)[NLD]) {      // outside the loop
      tab_factors(step, rs);
      store_lds(any_step(), buf, step, rc, ra, rs);
    };
    int32_t ti_c = 0, ti_a = 0;
    float tf = 0.f;
    if constexpr (GC || GA) {
      // pieces 0 and 1: the rows first - the addresses of the steps 0 and 1 wait for them - and the factors, which only
      // the LDS store of step 0 needs, behind the data requests
      int32_t t0c = 0, t0a = 0;
      tab_request(0, t0c, t0a);
      tab_request(1, ti_c, ti_a);
      tab_write_rows(0, t0c, t0a);
      tab_write_rows(1, ti_c, ti_a);
      float f0 = 0.f;
      tab_factor(t0c, f0);
      tab_factor(ti_c, tf);
      __syncthreads();
      tab_rows(0, nc, na);
      fetch(any_step(), 0, rc1, ra1);
      fetch(any_step(), cl(1), rc0, ra0);
      if constexpr (SC) {
        tab_write_factor(0, f0);
        tab_write_factor(1, tf);
        __syncthreads();
      }
    } else {
      fetch(any_step(), 0, rc1, ra1);
      fetch(any_step(), cl(1), rc0, ra0);
    }
    store_step(0, 0, rc1, ra1);
    __syncthreads();
    WT_STAMP(1);                                  // step 0 in LDS
    // entry of even local step t: buf0 = tile t, set0 = tile t+1, (nc, na) = the table rows of tile t+2.
    // The pair of steps (t, t + 1) fetches the steps t + 2 and t + 3 and stores t + 1 and t + 2.  stage: what it does for
    // the piece after the next one - 0 nothing, 1 request, 2 factor, 3 write, -1: the stage of the pair's place in its piece,
    // under branches (fp32)
    auto two_steps = [&](auto whole, auto stage, int t) {
      constexpr int ST = decltype(stage)::value;
      const int piece = (t >> 3) + 2, place = (t >> 1) & 3;
      if (ST == 1 || (ST < 0 && place == 0)) tab_request(piece, ti_c, ti_a);
      if (ST == 2 || (ST < 0 && place == 1)) tab_factor(ti_c, tf);
      fetch(whole, t + 2, rc1, ra1);
      tab_factors(t + 1, rs);
      __builtin_amdgcn_sched_barrier(0);
      WT_STAMP(2 + 4 * t);                        // loads issued
      compute(0);
      WT_STAMP(3 + 4 * t);                        // MFMAs issued
      store_lds(whole, 1, t + 1, rc0, ra0, rs);
      WT_STAMP(4 + 4 * t);                        // the step's data has arrived and is in LDS
      __syncthreads();
      WT_STAMP(5 + 4 * t);                        // barrier passed
      if (ST == 3 || (ST < 0 && place == 3)) {
        tab_write_rows(piece, ti_c, ti_a);
        tab_write_factor(piece, tf);
      }
      fetch(whole, t + 3, rc0, ra0);
      tab_factors(t + 2, rs);
      __builtin_amdgcn_sched_barrier(0);
      WT_STAMP(6 + 4 * t);
      compute(1);
      WT_STAMP(7 + 4 * t);
      store_lds(whole, 0, t + 2, rc1, ra1, rs);
      WT_STAMP(8 + 4 * t);
      __syncthreads();
      WT_STAMP(9 + 4 * t);
    };
    typedef std::integral_constant<int, 0> no_stage;
    // The steady part: while the steps up to t + 3 are whole (t + 3 < last); the fetches run two steps ahead of the
    // compute, so it ends two steps before the part does and at most one clamped pair and the remainder follow it.
    // 16-bit instances only: fp32 has NLD = 4, and its eight pointers go to scratch (+4 .. +12 bytes per lane over the
    // clamped loop, which already spills there), and so do the four unrolled pairs (+12); fp32 keeps the clamped forms for
    // every step and takes the table stages under branches.
    int t = 0;
    if constexpr (ES == 2) point_at(2);
    if constexpr ((GC || GA) && ES == 2) {        // whole pieces, all of their steps whole, with the table stages
      for (; t + 10 < nst; t += 8) {
        two_steps(whole_step(), std::integral_constant<int, 1>(), t);
        two_steps(whole_step(), std::integral_constant<int, 2>(), t + 2);
        two_steps(whole_step(), no_stage(), t + 4);
        two_steps(whole_step(), std::integral_constant<int, 3>(), t + 6);
      }
    }
    if constexpr (ES == 2)
      for (; t + 4 < nst; t += 2) two_steps(whole_step(), no_stage(), t);
    // (fp32 with a gather: ONE loop, staged to the end - a write happens in the fourth pair of a piece only, and if that pair
    // runs, the part's last step - all that clamped fetches read - lies in the next piece)
    typedef std::integral_constant<int, (GC || GA) && ES != 2 ? -1 : 0> tail_stage;
    for (; t + 3 < nst; t += 2) two_steps(any_step(), tail_stage(), t);
    const int rem = nst - t;
    if (rem == 3) {
      fetch(any_step(), t + 2, rc1, ra1);
      compute(0);
      store_step(1, t + 1, rc0, ra0);
      __syncthreads();
      compute(1);
      store_step(0, t + 2, rc1, ra1);
      __syncthreads();
      compute(0);
    } else if (rem == 2) {
      compute(0);
      store_step(1, t + 1, rc0, ra0);
      __syncthreads();
      compute(1);
    } else {
      compute(0);
    }
  }

  if (do_bias && lg == 0) {                       // every row of the ones-product is the column sum: take row 0
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) {
      const int n = n0 + wc * 64 + ni * 16 + li;
      if (n < p.N) wgrad_store_bias(p, acc_b[ni][0], slab_id, g, n);
    }
  }
  wgrad_store_tile(p, acc, slab_id, g, n0, k0, wr, wc, li, lg);
}

template <typename T, bool GC, bool GA, bool SC = false>
__global__ __launch_bounds__(WG_THREADS, 2) void wgrad_tn_kernel(const WgradDev p) {
  constexpr int ROWS = WgLds<T>::ROWS;
  const int tid = threadIdx.x;
  const int lane = tid & 63;

  // XCD-aware order: all tiles of one (group, split) read the SAME rows of dC and A (each byte is
  // needed by tiles_k resp. tiles_n workgroups), so they are given consecutive logical ids, which the
  // remap places on one XCD: the re-reads hit that XCD's L2 instead of the fabric.
  const int tiles = gridDim.x;
  int bz, gz;
  if (wgrad_ride_along(p, tid, bz, gz)) return;
  const int lin = blockIdx.x + tiles * (blockIdx.y + gridDim.y * bz);
  int tile, gs, g, sp, nst;
  int64_t r0, r1, s_begin;
  if (p.chunk_rows) {                          // gs = work unit; its slab is ws[gs]
    if (!wgrad_unit(p.group_offsets, p.G, p.chunk_rows, lin, tiles, lane, tile, gs, g, r0, r1)) return;
    sp = gs; s_begin = 0;
    nst = (int)((r1 - r0 + ROWS - 1) / ROWS);
  } else {
    const int log_id = xcd_remap(lin, tiles * gridDim.y * gz);
    tile = log_id % tiles; gs = log_id / tiles;
    g = gs % (int)gridDim.y; sp = gs / (int)gridDim.y;
    if (p.group_offsets && p.lpt) g = wgrad_lpt_group(p.group_offsets, p.G, g, lane);
    if (p.group_offsets) { r0 = p.group_offsets[g]; r1 = p.group_offsets[g + 1]; }
    else { r0 = 0; r1 = p.M; }
    const int64_t nsteps_all = (r1 - r0 + ROWS - 1) / ROWS;
    const int64_t per = (nsteps_all + p.splits - 1) / p.splits;
    s_begin = (int64_t)sp * per;
    int64_t s_end = s_begin + per;
    if (s_end > nsteps_all) s_end = nsteps_all;
    nst = (int)(s_end > s_begin ? s_end - s_begin : 0);
  }
  // slab / bias slab of this workgroup
  const int64_t slab_id = p.chunk_rows ? (int64_t)sp : (int64_t)sp * p.G + g;
  wgrad_tile_loop<T, GC, GA, SC>(p, tile, g, slab_id, r0, r1, s_begin, nst);
}

// the instances: every dtype with every pair of gathers; a per-row factor only on gathered dC rows
struct WgStaged {
  template <typename T, bool GC, bool GA, bool SC> static const void *instance() {
    if constexpr (!SC || GC) return (const void *)wgrad_tn_kernel<T, GC, GA, SC>;
    else return nullptr;
  }
};

int launch_wgrad_staged(int dtype, bool gc, bool ga, bool sc, dim3 grid, const WgradDev &d, hipStream_t s) {
  // the two operand images of both buffers and, for the instances that gather, the table behind them: 36 / 66 KiB (16-bit /
  // fp32) + 6 KiB, two workgroups per CU in either case
  const size_t lds16 = 4 * WgLds<half_t>::ROWS * WgLds<half_t>::STRIDE, lds32 = 4 * WgLds<float>::ROWS * WgLds<float>::STRIDE;
  static_assert(2 * (4 * WgLds<float>::ROWS * WgLds<float>::STRIDE + WG_TAB_BYTES) <= 160 * 1024, "two workgroups per CU");
  static bool attr_set = false;
  if (!attr_set) {                               // the fp32 images exceed the 64 KiB a launch gets without asking
    wgrad_each_instance<WgStaged>([&](int dt, bool, bool, bool, const void *k) {
      (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)((dt == M3_F32 ? lds32 : lds16) + WG_TAB_BYTES));
    });
    attr_set = true;
  }
  const size_t lds = (dtype == M3_F32 ? lds32 : lds16) + (gc || ga ? WG_TAB_BYTES : 0);
  return wgrad_launch_instance<WgStaged>(dtype, gc, ga, sc, grid, dim3(WG_THREADS), lds, d, s);
}

}  // namespace m3

#ifdef M3_WGRAD_STAMPS
extern "C" int m3_debug_wtn_stamps(unsigned long long *dst, int wgs, int clear) {
  using namespace m3;
  if (wgs > WTSTAMP_WGS) wgs = WTSTAMP_WGS;
  const size_t bytes = (size_t)wgs * WTSTAMP_N * sizeof(unsigned long long);
  if (dst && hipMemcpyFromSymbol(dst, HIP_SYMBOL(g_wtn_stamps), bytes) != hipSuccess) return M3_ERR_LAUNCH;
  if (clear) {
    void *sym = nullptr;
    if (hipGetSymbolAddress(&sym, HIP_SYMBOL(g_wtn_stamps)) != hipSuccess || hipMemset(sym, 0, sizeof(g_wtn_stamps)) != hipSuccess) return M3_ERR_LAUNCH;
  }
  return M3_OK;
}
#endif
