// The statements of the attention backward kernels (bert_encoder_bwd.hip: k_bert_attention_bwd and its sibling with the
// relative bias), included INSIDE each kernel's braces so that both are compiled from one text and the kernel without a
// bias keeps the instructions it had before the sibling existed (an inlined device function does not: the compiler
// schedules its address arithmetic differently).  Expects in scope: the template parameters DH and DROP, a
// `constexpr bool BIAS`, and qkv, rel_bias (read with BIAS only), dctx, T, heads, keep, keep_scale, dqkv, sq.
  extern __shared__ __attribute__((aligned(16))) float smem[];
  constexpr int LD = DH + 1;
  const int b = blockIdx.x / heads, h = blockIdx.x % heads;
  const int H = heads * DH;
  const int tid = threadIdx.x, nthr = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nthr >> 6;
  float* ks = smem;                                   // [T, LD]
  float* vs = ks + T * LD;                            // [T, LD]
  float* qs = vs + T * LD;                            // [T, LD]
  float* gs = qs + T * LD;                            // [T, LD]  dO
  float* bs = gs + T * LD;                            // [2T - 1] the head's bias row (BIAS only; 2T floats reserved)
  float* ds = BIAS ? bs + 2 * T + wave * kBertMaxT    // [kBertMaxT]  this wave's row of dS
                   : gs + T * LD + wave * kBertMaxT;
  float* dsg = sq + (size_t)blockIdx.x * 2 * T * T;   // [T, T]  dS, query row i, key column j
  float* ptg = dsg + (size_t)T * T;                   // [T, T]  pt

  const float* base = qkv + (size_t)b * T * 3 * H + h * DH;
  const float* gbase = dctx + (size_t)b * T * H + h * DH;
  float* obase = dqkv + (size_t)b * T * 3 * H + h * DH;
  for (int i = tid; i < T * (DH / 4); i += nthr) {
    const int j = i / (DH / 4), c = (i % (DH / 4)) * 4;
    const float* row = base + (size_t)j * 3 * H;
    const f32x4 qv = *(const f32x4*)(row + c);
    const f32x4 kv = *(const f32x4*)(row + H + c);
    const f32x4 vv = *(const f32x4*)(row + 2 * H + c);
    const f32x4 gv = *(const f32x4*)(gbase + (size_t)j * H + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      qs[j * LD + c + e] = qv[e];
      ks[j * LD + c + e] = kv[e];
      vs[j * LD + c + e] = vv[e];
      gs[j * LD + c + e] = gv[e];
    }
  }
  if (BIAS) {
    const float* br = rel_bias + (size_t)h * (2 * T - 1);
    for (int i = tid; i < 2 * T - 1; i += nthr) bs[i] = br[i];
  }
  __syncthreads();

  const float scale = 1.f / sqrtf((float)DH);
  const int j0 = lane, j1 = lane + 64;
  for (int t = wave; t < T; t += nw) {
    const float* q = qs + t * LD;
    const float* go = gs + t * LD;
    float s0 = -INFINITY, s1 = -INFINITY, dp0 = 0.f, dp1 = 0.f;
    if (j0 < T) {
      const float *k = ks + j0 * LD, *v = vs + j0 * LD;
      float a = 0.f, c = 0.f;
#pragma unroll
      for (int d = 0; d < DH; ++d) {
        a = fmaf(q[d], k[d], a);
        c = fmaf(go[d], v[d], c);
      }
      s0 = a * scale;
      dp0 = c;
    }
    if (j1 < T) {
      const float *k = ks + j1 * LD, *v = vs + j1 * LD;
      float a = 0.f, c = 0.f;
#pragma unroll
      for (int d = 0; d < DH; ++d) {
        a = fmaf(q[d], k[d], a);
        c = fmaf(go[d], v[d], c);
      }
      s1 = a * scale;
      dp1 = c;
    }
    if (BIAS) {  // in blocks of their own: the two blocks above are those of the kernel without a bias
      if (j0 < T) s0 = bert_att_opaque(s0) + bs[j0 - t + T - 1];
      if (j1 < T) s1 = bert_att_opaque(s1) + bs[j1 - t + T - 1];
    }
    const float m = wave_max(fmaxf(s0, s1));
    const float e0 = j0 < T ? expf(s0 - m) : 0.f, e1 = j1 < T ? expf(s1 - m) : 0.f;
    const float sum = wave_sum(e0 + e1);
    const float p0 = e0 / sum, p1 = e1 / sum;
    float m0 = 1.f, m1 = 1.f;
    if (DROP) {
      const uint8_t* kr = keep + ((size_t)blockIdx.x * T + t) * T;     // blockIdx.x = b heads + h
      m0 = j0 < T && kr[j0] ? keep_scale : 0.f;
      m1 = j1 < T && kr[j1] ? keep_scale : 0.f;
    }
    const float pt0 = DROP ? p0 * m0 : p0, pt1 = DROP ? p1 * m1 : p1;
    const float r = wave_sum(fmaf(pt0, dp0, pt1 * dp1));
    // the masked product is rounded on its own (behind bert_att_opaque it cannot be fused into the subtraction): with
    // one key p = 1, r is that same rounded product and dS is exactly 0, as it is in exact arithmetic
    const float dS0 = p0 * ((DROP ? bert_att_opaque(dp0 * m0) : dp0) - r);
    const float dS1 = p1 * ((DROP ? bert_att_opaque(dp1 * m1) : dp1) - r);
    if (j0 < T) {
      ds[j0] = dS0;
      dsg[t * T + j0] = dS0;
      ptg[t * T + j0] = pt0;
    }
    if (j1 < T) {
      ds[j1] = dS1;
      dsg[t * T + j1] = dS1;
      ptg[t * T + j1] = pt1;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane < DH) {
      float acc = 0.f;
      for (int j = 0; j < T; ++j) acc = fmaf(ds[j], ks[j * LD + lane], acc);
      obase[(size_t)t * 3 * H + lane] = acc * scale;
    }
    // the next row's writes to ds follow this row's reads in program order (one wave, LDS in order)
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();          // the squares are written by this workgroup and read by it: visible behind the barrier

  for (int idx = tid; idx < T * DH; idx += nthr) {
    const int j = idx / DH, d = idx % DH;
    float ak = 0.f, av = 0.f;
    for (int i = 0; i < T; ++i) {
      ak = fmaf(dsg[i * T + j], qs[i * LD + d], ak);
      av = fmaf(ptg[i * T + j], gs[i * LD + d], av);
    }
    obase[(size_t)j * 3 * H + H + d] = ak * scale;
    obase[(size_t)j * 3 * H + 2 * H + d] = av;
  }
