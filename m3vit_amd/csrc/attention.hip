// Fused (flash-style) multi-head attention forward / backward for gfx950 on the packed
// qkv activations of the ViT block:  o = softmax(q k^T * dh^-0.5) v.
//
// Replaces Attention.forward's q@k^T -> softmax -> @v chain and its autograd
// (models/moe/ckpt/vision_transformer_moe.py:299-313; dense twin
// models/backbones/vit.py:177-207) without materialising the [B,h,N,N] scores.
// qkv is exactly what the qkv Linear wrote: [token][3][head][dh]; o is [token][head*dh].
//
// This file holds the C entry points and what they share; the kernels are picked by dtype and N:
//   fp32                         attention_f32.hip   exact 16x16x4 f32 MFMA, any N
//   fp16 / bf16, N <= ATTN_KEYS  attention_b16.hip   LDS-resident kernels
//   fp16 / bf16, N >  ATTN_KEYS  attention_b16.hip   streamed kernels
// A backward over more than one key block (N > ATTN_KEYS, any dtype) leaves dQ as one fp32 slab per key block
// (attention_dev.h); attention_dq_reduce_kernel sums them into dqkv.
#include "attention_dev.h"

namespace m3 {

// dq[b, n, h, :] = sum over key blocks of the fp32 slabs (key-block order), written into the q slot of dqkv
template <typename T>
__global__ void attention_dq_reduce_kernel(const float *__restrict__ ws, int nkb, int B, int N, int heads, int DH,
                                           T *__restrict__ dqkv) {
  const int64_t per = (int64_t)B * heads * N * DH;
  const int64_t i4 = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * 4;
  if (i4 >= per) return;
  f32x4 s = *(const f32x4 *)(ws + i4);
  for (int kb = 1; kb < nkb; ++kb) s += *(const f32x4 *)(ws + kb * per + i4);
  const int d = (int)(i4 % DH);
  const int64_t row = i4 / DH;                  // (b*heads + h)*N + n
  const int n = (int)(row % N);
  const int64_t bh = row / N;
  const int h = (int)(bh % heads);
  const int64_t b = bh / heads;
  Vec4<T>::store(dqkv + ((b * N + n) * 3) * (int64_t)(heads * DH) + h * DH + d, s);
}

template <typename T>
static void launch_dq_reduce_t(const float *dq_ws, int B, int N, int heads, int dh, void *dqkv, hipStream_t s) {
  const int64_t n4 = (int64_t)B * heads * N * dh / 4;
  hipLaunchKernelGGL((attention_dq_reduce_kernel<T>), dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, dq_ws,
                     attn_key_blocks(N), B, N, heads, dh, (T *)dqkv);
}

static int launch_dq_reduce(int dtype, const float *dq_ws, int B, int N, int heads, int dh, void *dqkv, hipStream_t s) {
  if (dtype == M3_BF16) launch_dq_reduce_t<bf16_t>(dq_ws, B, N, heads, dh, dqkv, s);
  else if (dtype == M3_F16) launch_dq_reduce_t<half_t>(dq_ws, B, N, heads, dh, dqkv, s);
  else launch_dq_reduce_t<float>(dq_ws, B, N, heads, dh, dqkv, s);
  return check_launch("m3_attention_bwd(dq reduce)");
}

}  // namespace m3

using namespace m3;

extern "C" int m3_attention_fwd(const void *qkv, int dtype, int B, int N, int heads, int dh, void *o, float *lse,
                                void *stream) {
  M3_REQUIRE(qkv && o && lse, "m3_attention_fwd: null operand");
  M3_REQUIRE(dtype_ok(dtype), "m3_attention_fwd: bad dtype");
  M3_REQUIRE(dh == 32 || dh == 64, "m3_attention_fwd: head dim %d not in {32, 64}", dh);
  M3_REQUIRE(B > 0 && N > 0 && heads > 0, "m3_attention_fwd: bad shape");
  M3_REQUIRE(((uintptr_t)qkv % 16) == 0 && ((uintptr_t)o % 16) == 0, "m3_attention_fwd: alignment");
  const float scale = 1.0f / sqrtf((float)dh);
  hipStream_t s = (hipStream_t)stream;
  switch (attn_family(dtype, N)) {
    case ATTN_F32: return launch_attention_fwd_f32(qkv, B, N, heads, dh, o, lse, scale, s);
    case ATTN_RES: return launch_attention_fwd_res(dtype, qkv, B, N, heads, dh, o, lse, scale, s);
    default: return launch_attention_fwd_stream(dtype, qkv, B, N, heads, dh, o, lse, scale, s);
  }
}

extern "C" int m3_attention_plan(int dtype, int N, int dh, m3_attention_plan_out *p) {
  M3_REQUIRE(p, "m3_attention_plan: null output");
  M3_REQUIRE(dtype_ok(dtype), "m3_attention_plan: bad dtype");
  M3_REQUIRE(dh == 32 || dh == 64, "m3_attention_plan: head dim %d not in {32, 64}", dh);
  M3_REQUIRE(N > 0, "m3_attention_plan: bad N");
  const AttnFamily f = attn_family(dtype, N);
  *p = m3_attention_plan_out{};
  p->fwd_family = p->bwd_family = f == ATTN_F32 ? M3_ATTN_F32 : f == ATTN_RES ? M3_ATTN_RESIDENT : M3_ATTN_STREAMED;
  p->fwd_key_tiles = f == ATTN_RES ? attn_res_fwd_nkt(N) : 0;
  p->bwd_tiles_per_wave = f == ATTN_RES ? attn_res_bwd_kte(N, dh) : 0;
  p->bwd_key_blocks = attn_key_blocks(N);
  return M3_OK;
}

extern "C" int64_t m3_attention_bwd_ws_elems(int B, int N, int heads, int dh) {
  return N > ATTN_KEYS ? attn_bwd_ws(B, N, heads, dh).elems : 0;
}

extern "C" int m3_attention_bwd(const void *qkv, const void *o, const void *d_o, const float *lse, int dtype, int B,
                                int N, int heads, int dh, void *dqkv, float *dq_ws, void *stream) {
  M3_REQUIRE(qkv && o && d_o && lse && dqkv, "m3_attention_bwd: null operand");
  M3_REQUIRE(dtype_ok(dtype), "m3_attention_bwd: bad dtype");
  M3_REQUIRE(dh == 32 || dh == 64, "m3_attention_bwd: head dim %d not in {32, 64}", dh);
  M3_REQUIRE(N > 0, "m3_attention_bwd: bad N");
  M3_REQUIRE(N <= ATTN_KEYS || dq_ws, "m3_attention_bwd: N=%d > %d needs the fp32 dQ workspace (m3_attention_bwd_ws_elems)", N, ATTN_KEYS);
  if (N <= ATTN_KEYS) dq_ws = nullptr;
  const float scale = 1.0f / sqrtf((float)dh);
  hipStream_t s = (hipStream_t)stream;
  const AttnFamily f = attn_family(dtype, N);
  if (f == ATTN_RES) return launch_attention_bwd_res(dtype, qkv, o, d_o, lse, B, N, heads, dh, dqkv, scale, s);
  const int rc = f == ATTN_F32 ? launch_attention_bwd_f32(qkv, o, d_o, lse, B, N, heads, dh, dqkv, dq_ws, scale, s)
                                 : launch_attention_bwd_stream(dtype, qkv, o, d_o, lse, B, N, heads, dh, dqkv, dq_ws, scale, s);
  if (rc || N <= ATTN_KEYS) return rc;
  return launch_dq_reduce(dtype, dq_ws, B, N, heads, dh, dqkv, s);
}
