// Masked attention (sf_maskattn.hip) as the mask decoder's launch sequence (sf_maskdec.hip) reaches it: the forward's arguments and its
// launcher.  The kernels, the backward and every sf_op_maskattn_* / sf_op_maskdec_attention entry point are in sf_maskattn.hip.
#pragma once
#include "sf_common.h"

// what the forward and the backward read alike, and what the shared device pieces of sf_maskattn.hip take
struct SfMkaCore {
  const float* q; const float* k; const float* v;      // fp32 rows; a head's columns at h * hd
  const uint32_t* mask;                                // [F, (heads,) Tq, words], bit j & 31 of word j / 32 set: key j hidden; or null
  int q_pitch, kv_pitch;                               // elements per row; K and V rows have one pitch
  int F, Tq, Tk, heads, hd, words, no_skip;
  int mask_per_head;                                   // the mask is [F, heads, Tq, words] (training only)
  float scale;
};

struct SfMkaFwd : SfMkaCore {
  const float* kpos;                                   // [Tk, pos_pitch] by key, added to K; or null
  float* ctx; bf16_t* ctx_hi; bf16_t* ctx_lo;          // [F Tq, heads * hd]; any of them null
  int pos_pitch;
  // the training forward (sf_op_maskattn_forward) only; without it and without mask_per_head the kernel is the instance the decoder runs
  float* stats;                                        // [F, heads, Tq]: log-sum-exp of the scaled scores over the visible keys, +inf without one
};

// every pointer 16-byte aligned (planes 8, mask and stats 4), pitches multiples of 4, hd % 8 == 0 in 8..128: checked there
hipError_t mka_launch_forward(const SfMkaFwd& p, hipStream_t s);
