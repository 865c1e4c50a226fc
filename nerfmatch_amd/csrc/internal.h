// Functions that cross translation units without being part of the C API (include/nerfmatch_amd.h).  Declared here once and included
// by the defining and the calling file, so a drifted signature is a compile error, not an unresolved symbol at load time.
#pragma once
#include "common.h"

// gemm.hip / gemm_bf16.hip -> match.hip: sim[M,N] = mask_fill(scale * im[M,C] . pt[N,C]^T); the split-bf16 form packs pt into `blob`
// (nm_linear_blob_bytes_bf16x3(N, C) bytes of workspace) first and needs N % 8 == 0, C % 8 == 0
int nm_internal_sim(const float* im, const float* pt, int M, int N, int C, float scale, const uint8_t* im_mask, const uint8_t* pt_mask,
                    float* sim, hipStream_t s);
int nm_internal_sim_bf16x3(const float* im, const float* pt, int M, int N, int C, float scale, const uint8_t* im_mask,
                           const uint8_t* pt_mask, float* sim, void* blob, hipStream_t s);

// attention_v2.hip -> attention.hip: the split-bf16 forward (pre-split of K / V into `workspace`, then attn32_v3_kernel)
size_t nm_internal_attn_v2_workspace(int B, int S, int heads);
int nm_internal_attn_v2(const float* q, const float* k, const float* v, int ldq, int ldk, int ldv, int B, int L, int S, int heads,
                        float scale, void* workspace, float* out, hipStream_t s, float* nlse_out);

// attention_bwd_v2.hip -> attention_bwd.hip: the split-bf16 backward
size_t nm_internal_attn_bwd_v2_workspace(int B, int L, int S, int heads);
int nm_internal_attn_bwd_v2(const float* q, const float* k, const float* v, const float* o, const float* d_o, int ldq, int ldk, int ldv,
                            int ldo, int lddo, int B, int L, int S, int heads, float scale, float* dq, float* dk, float* dv, int lddq,
                            int lddk, int lddv, void* workspace, hipStream_t s, const float* nlse_fwd);
