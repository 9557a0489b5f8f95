// Definitions shared by the attention sources (attention.hip: entry points, dispatch and the dQ slab reduction;
// attention_f32.hip: exact-fp32 kernels; attention_b16.hip: fp16 / bf16 kernels): the key block, the layout of the
// backward workspace and the launchers that attention.hip dispatches to.
#pragma once
#include "common.h"

namespace m3 {

// Keys per workgroup of every backward kernel (one key block), and therefore the longest sequence that the
// LDS-resident 16-bit kernels take and the longest one whose backward needs no workspace.
constexpr int ATTN_KEYS = 256;
static inline int attn_key_blocks(int N) { return (N + ATTN_KEYS - 1) / ATTN_KEYS; }

// fp32 workspace of a backward over more than one key block: the dQ slabs [key block][B*heads][N][dh], summed in
// key-block order by attention_dq_reduce_kernel, followed by delta [B*N*heads] (16-bit streamed kernel only).
struct AttnBwdWs { int64_t delta_off, elems; };
static inline AttnBwdWs attn_bwd_ws(int B, int N, int heads, int dh) {
  const int64_t slabs = (int64_t)attn_key_blocks(N) * B * heads * N * dh;
  return AttnBwdWs{slabs, slabs + (int64_t)B * N * heads};
}

// Which family of kernels takes a call (attention.hip dispatches by it, m3_attention_plan reports it), and the template
// instance of the LDS-resident 16-bit kernels (attention_b16.hip launches by them)
enum AttnFamily { ATTN_F32, ATTN_RES, ATTN_STREAM };
static inline AttnFamily attn_family(int dtype, int N) { return dtype == M3_F32 ? ATTN_F32 : N <= ATTN_KEYS ? ATTN_RES : ATTN_STREAM; }
static inline int attn_res_fwd_nkt(int N) { return ((N + 15) / 16 + 3) / 4 * 4; }      // key tiles rounded up to 4, 8, 12, 16
// tiles per wave of the LDS-resident backward for N keys: ceil(key tiles / waves)
static inline int attn_res_bwd_kte(int N, int dh) { const int nw = dh == 32 ? 4 : 8; return ((N + 15) / 16 + nw - 1) / nw; }

// attention_f32.hip
int launch_attention_fwd_f32(const void *qkv, int B, int N, int heads, int dh, void *o, float *lse, float scale, hipStream_t s);
int launch_attention_bwd_f32(const void *qkv, const void *o, const void *d_o, const float *lse, int B, int N, int heads, int dh,
                             void *dqkv, float *dq_ws, float scale, hipStream_t s);
// attention_b16.hip: dtype is M3_F16 or M3_BF16; _res needs N <= ATTN_KEYS, _stream is meant for longer sequences
int launch_attention_fwd_res(int dtype, const void *qkv, int B, int N, int heads, int dh, void *o, float *lse, float scale,
                             hipStream_t s);
int launch_attention_fwd_stream(int dtype, const void *qkv, int B, int N, int heads, int dh, void *o, float *lse, float scale,
                                hipStream_t s);
int launch_attention_bwd_res(int dtype, const void *qkv, const void *o, const void *d_o, const float *lse, int B, int N, int heads,
                             int dh, void *dqkv, float scale, hipStream_t s);
int launch_attention_bwd_stream(int dtype, const void *qkv, const void *o, const void *d_o, const float *lse, int B, int N, int heads,
                                int dh, void *dqkv, float *dq_ws, float scale, hipStream_t s);

}  // namespace m3
