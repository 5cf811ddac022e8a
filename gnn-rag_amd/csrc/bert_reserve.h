// The reserve of the encoder layers' saving forward (gnnrag_bert_layers_forward_save, bert_encoder.hip) as the backward
// (bert_encoder_bwd.hip) reads it: per layer, in this order and without padding between the blocks (H % 4 == 0 and
// I % 4 == 0 keep every block 16-byte aligned), M = B T rows each:
//   xin  [M, H]   the layer's input
//   qkv  [M, 3H]  the packed query / key / value rows
//   ctx  [M, H]   the attention output
//   sum1 [M, H]   the attention output projection in front of LayerNorm 1: dense + bias under hidden dropout (the residual
//                 is added behind the dropout), dense + bias + residual without it
//   x1   [M, H]   LayerNorm 1's output
//   pre  [M, I]   the FFN pre-activation (the value in front of the GELU)
//   sum2 [M, H]   the FFN output projection in front of LayerNorm 2, as sum1
// (8 H + I) 4 bytes per row and layer.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace gnnrag {

struct BertReserve {
  size_t xin, qkv, ctx, sum1, x1, pre, sum2, layer;   // byte offsets inside a layer's block, and the block's size
};

static inline BertReserve bert_reserve(int64_t M, int64_t H, int64_t I) {
  BertReserve r;
  const size_t mh = (size_t)M * H * sizeof(float), mi = (size_t)M * I * sizeof(float);
  r.xin = 0;
  r.qkv = r.xin + mh;
  r.ctx = r.qkv + 3 * mh;
  r.sum1 = r.ctx + mh;
  r.x1 = r.sum1 + mh;
  r.pre = r.x1 + mh;
  r.sum2 = r.pre + mi;
  r.layer = r.sum2 + mh;
  return r;
}

// The embedding reserve (gnnrag_bert_embed_forward_save, read by gnnrag_bert_embed_backward), without padding:
//   sum0 [M, H]   the row in front of the embedding LayerNorm: word + type + position
//   pos  [M]      int32: the position row of each token; -1 for a token whose id or position lies outside its table
// (H + 1) 4 bytes per row.
struct BertEmbedReserve {
  size_t sum0, pos, total;
};

static inline BertEmbedReserve bert_embed_reserve(int64_t M, int64_t H) {
  BertEmbedReserve r;
  r.sum0 = 0;
  r.pos = (size_t)M * H * sizeof(float);
  r.total = r.pos + (size_t)M * sizeof(int32_t);
  return r;
}

}  // namespace gnnrag
