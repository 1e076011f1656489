// Launcher of the CIDEr / CIDEr-D reward over token ids (csrc/cider_reward.hip; C-ABI kmb_cider_reward): one score per row of a
// [B, L] id matrix against reference tables resident in device memory (src/rewards.py builds them), one launch, no host
// synchronisation.  DESIGN.md section 6r.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

constexpr int KMB_CIDER_MAX_T = 256;    // columns of the id matrix: the kernel gives every column one lane and holds the row in LDS
constexpr int KMB_CIDER_ORDERS = 4;     // n-gram orders 1..4
constexpr int KMB_CIDER_VARIANT_D = 0;      // clipped numerator, Gaussian length penalty
constexpr int KMB_CIDER_VARIANT_PLAIN = 1;  // plain tf-idf cosine, no penalty

// The tables of build_cider_tables (src/rewards.py), all on the device but df_offsets, which is read on the host at the call.
struct KmbCiderTables {
  int n_items;                       // N
  const uint64_t* df_keys;           // [df_offsets[4]] packed n-grams, ascending UNSIGNED within each order's slice
  const float* df_idf;               // [df_offsets[4]] log N - log max(1, df)
  int64_t df_offsets[KMB_CIDER_ORDERS + 1];
  float idf_miss;                    // float32(log N): the idf of an n-gram no reference holds
  const int32_t* item_ref_offsets;   // [N + 1] item i's references are [item_ref_offsets[i], item_ref_offsets[i + 1])
  int n_refs;                        // R
  const int32_t* ref_len;            // [R] tokens of a reference
  const float* ref_norm;             // [R, 4] ||g_r,n||
  const int32_t* ref_ng_offsets;     // [4 R + 1] slice 4 r + (n - 1) of ref_keys / ref_w
  const uint64_t* ref_keys;          // ascending unsigned within each (reference, order) slice
  const float* ref_w;                // count * idf
  int64_t n_ref_entries;             // ref_ng_offsets[4 R]
};

// The argument checks of kmb_cider_reward (capi_ops.cpp): null pointers, L > KMB_CIDER_MAX_T, B < 0, sigma <= 0, an unknown variant.
int kmb_cider_reward_validate(const char* who, const int64_t* ids, int ld, int B, int L, const int32_t* item_of_row,
                              const KmbCiderTables& t, int variant, float sigma, const float* out);

// One workgroup per row b < B of ids [B, ld] (int64, L columns read): out[b] = the row's score against the references of item
// item_of_row[b].  Arguments as kmb_cider_reward (include/kmbart.h), already validated.
hipError_t kmb_cider_reward_launch(const int64_t* ids, int ld, int B, int L, int pad_token, int bos_token, int eos_token,
                                   const int32_t* item_of_row, const KmbCiderTables& t, int variant, float sigma, float* out,
                                   hipStream_t stream);
