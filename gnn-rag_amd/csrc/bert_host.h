// Host-side rules of the BERT-class encoder shared by its forward entries (bert_encoder.hip) and its backward
// (bert_encoder_bwd.hip): the limits the kernels are written for, the shape and scale rules of the entry points, the
// per-layer pointer check and the addressing of the keep planes.  One definition each: an entry point added later
// answers the same arguments with the same codes.  The reserve's layout is bert_reserve.h.
#pragma once
#include <cmath>

#include "bert_reserve.h"
#include "gnnrag_common.h"

namespace gnnrag {

constexpr int kBertMaxT = 128;       // keys per question: two per lane
constexpr int kBertLnRows = 4;       // rows (waves) per workgroup of the LayerNorm kernels
// rows B T of gnnrag_bert_embed_backward: its scatter compares every row's id with every other's (M M / 64 ballots)
constexpr int64_t kBertEmbedBwdMaxRows = 65536;

// the shapes the attention kernels (forward and backward) take
static inline bool bert_att_shape_ok(int64_t B, int32_t T, int32_t heads, int32_t dh) {
  return (dh == 32 || dh == 64) && T >= 1 && T <= kBertMaxT && heads >= 1 && B >= 1 && B * heads < ((int64_t)1 << 31);
}

// the scale of a mask that is given: finite and > 0 (1 / (1 - p) of a p < 1); that of a NULL mask is not read
static inline bool bert_scale_ok(const uint8_t* keep, float scale) { return !keep || (std::isfinite(scale) && scale > 0.f); }

// Which fields of a gnnrag_bert_layer an entry point reads: bit i is field i in the struct's order.  The forward entries
// read all 12; the backward reads the four weights and the two LayerNorm gains (a NULL bias is legal there).
constexpr unsigned kBertFieldsAll = 0xfffu;
constexpr unsigned kBertFieldsBwd = 0x555u;   // W_qkv, W_o, ln1_g, W_i, W_f, ln2_g

// One layer's pointers: any NULL among `fields` is GNNRAG_E_BADARG before any misaligned one is GNNRAG_E_UNSUPPORTED.
static inline int bert_layer_ptrs_check(const gnnrag_bert_layer& y, unsigned fields) {
  const float* const p[12] = {y.W_qkv, y.b_qkv, y.W_o, y.b_o, y.ln1_g, y.ln1_b, y.W_i, y.b_i, y.W_f, y.b_f, y.ln2_g, y.ln2_b};
  for (int i = 0; i < 12; ++i)
    if ((fields >> i & 1u) && !p[i]) return GNNRAG_E_BADARG;
  for (int i = 0; i < 12; ++i)
    if ((fields >> i & 1u) && !aligned16(p[i])) return GNNRAG_E_UNSUPPORTED;
  return 0;
}

// The keep bytes of one call (gnnrag_bert_keep_hidden_bytes / _att_bytes): hidden plane 0 is the embedding output's,
// plane 1 + 2l layer l's attention output projection, plane 2 + 2l its FFN output projection, M H bytes each; attention
// plane l is layer l's probabilities, B heads T T bytes.  A NULL buffer gives NULL planes: that site keeps everything.
struct BertKeep {
  const uint8_t *hidden, *att;
  size_t plane, att_plane;
  BertKeep(const uint8_t* keep_hidden, const uint8_t* keep_att, int64_t B, int32_t T, int32_t H, int32_t heads)
      : hidden(keep_hidden), att(keep_att), plane((size_t)B * T * H), att_plane((size_t)B * heads * T * T) {}
  const uint8_t* att_out(int l) const { return hidden ? hidden + (size_t)(1 + 2 * l) * plane : nullptr; }
  const uint8_t* ffn_out(int l) const { return hidden ? hidden + (size_t)(2 + 2 * l) * plane : nullptr; }
  const uint8_t* probs(int l) const { return att ? att + (size_t)l * att_plane : nullptr; }
};

}  // namespace gnnrag
