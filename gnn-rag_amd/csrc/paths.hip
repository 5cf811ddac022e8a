// Reasoning paths on the device: the retrieval step of GNN-RAG (DESIGN.md "Reasoning paths").
//
// The reference joins every question entity to every retrieved candidate by ALL shortest paths of the question's
// subgraph, seen as a simple undirected graph (llm/src/utils/graph_utils.py: build_graph + get_truth_paths, called from
// llm/src/qa_prediction/build_qa_input.py:114-127): a networkx graph per question, nx.all_shortest_paths per pair.
// Here the graph is derived once from the batch structure that is already on the device (gnnrag_ugraph_build) and one
// call (gnnrag_shortest_paths) turns (seed flags, candidate lists of gnnrag_topp_candidates) into paths:
//
//   k_ug_emit / sort / k_ug_heads / scan / k_ug_compact / k_ug_ptr   the simple undirected adjacency
//   k_paths_bfs      one workgroup per (question, seed): levels + number of shortest paths, pull-based, no atomics
//   k_paths_offsets  exclusive scan of min(n_paths, max_paths) over the pairs
//   k_paths_unrank   one lane per written path: rank -> path
//
// The second path set of the reference, the rule-guided walks (graph_utils.py: bfs_with_rule, called by apply_rules of
// build_qa_input.py), runs on the same adjacency (gnnrag_rule_paths):
//
//   k_rule_edge_rel  relation of every adjacency record (that of its winning fact), staged once per call
//   k_rule_counts    one workgroup per (question, rule): down_l[v] = walks from v that complete the rule from hop l on,
//                    levels L-1 .. 0; then n_paths = down_0[seed] for every seed of the question
//   k_rule_offsets   the scan of k_paths_offsets over min(n_paths, max_paths)
//   k_rule_unrank    one lane per written walk: rank -> walk, node sequence ascending from the seed outwards
//
// Integer work only; every sum has one fixed order (and the saturating add of non-negative counts is associative), so
// results are bit-reproducible and do not depend on where a question sits in its batch.
#include "gnnrag_common.h"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

namespace gnnrag {

constexpr int kPathThreads = 512;          // k_paths_bfs: 8 waves per (question, seed)
constexpr int kPathLaneDeg = 32;           // rows with more neighbours are scanned by a wave instead of a lane
constexpr int kPathHubCap = 4096;          // wave-scanned rows per question (further ones fall back to a lane)
constexpr int kPathMaxN = 65536;           // levels are bytes in LDS
constexpr int kPathMaxHops = 254;          // level 255 = not reached
constexpr unsigned kSigmaMax = 0x7fffffffu;
constexpr unsigned kUnvisited = 255u;
constexpr size_t kPathLdsFixed = 16 + kPathThreads * 4 + (size_t)kPathHubCap * 4;

__device__ __forceinline__ unsigned sat_add(unsigned a, unsigned b) {      // a, b <= kSigmaMax: no wrap
  const unsigned s = a + b;
  return s > kSigmaMax ? kSigmaMax : s;
}

// workgroup-wide OR through a flag in the dynamic LDS region (no static LDS in front of it: the kernel's dynamic cap is
// raised to the CU's whole LDS); the barriers also order the round's LDS / global writes before the next round's reads
__device__ __forceinline__ int block_or(int pred, int32_t* flag) {
  __syncthreads();
  if (threadIdx.x == 0) *flag = 0;
  __syncthreads();
  if (pred) *flag = 1;
  __syncthreads();
  return *flag;
}

// ---- adjacency ---------------------------------------------------------------------------------------------------------
static unsigned node_bits(size_t BN) {       // bits that hold the values 0 .. BN (BN itself = the "dropped" key)
  unsigned bits = 1;
  while (bits < 32 && ((size_t)1 << bits) <= BN) ++bits;
  return bits;
}

static size_t ug_sort_temp_bytes(size_t n, unsigned end_bit) {
  size_t bytes = 0;
  const unsigned long long* kin = nullptr;
  unsigned long long* kout = nullptr;
  const int32_t* vin = nullptr;
  int32_t* vout = nullptr;
  hipError_t e = rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, n, 0u, end_bit, (hipStream_t)0, false);
  if (e != hipSuccess || bytes == 0) {
    (void)hipGetLastError();
    bytes = (size_t)32 * (n > 0 ? n : 1) + ((size_t)1 << 20);      // conservative bound (no device to ask)
  }
  return bytes;
}

static size_t ug_scan_temp_bytes(size_t n) {
  size_t bytes = 0;
  const int32_t* in = nullptr;
  int32_t* out = nullptr;
  hipError_t e = rocprim::exclusive_scan(nullptr, bytes, in, out, (int32_t)0, n, rocprim::plus<int32_t>(), (hipStream_t)0,
                                         false);
  if (e != hipSuccess || bytes == 0) {
    (void)hipGetLastError();
    bytes = (size_t)8 * (n > 0 ? n : 1) + ((size_t)1 << 20);
  }
  return bytes;
}

struct UgScratch {
  size_t key_in, key_out, val_in, val_out, flag, scan, temp, temp_bytes, total;
};

static UgScratch ug_scratch_layout(int64_t F, int32_t B, int32_t N) {
  UgScratch L;
  const size_t n = 2 * (size_t)(F > 0 ? F : 1);
  Carve cv;
  L.key_in = cv.take(n * 8);
  L.key_out = cv.take(n * 8);
  L.val_in = cv.take(n * 4);
  L.val_out = cv.take(n * 4);
  L.flag = cv.take(n * 4);
  L.scan = cv.take(n * 4);
  const size_t a = ug_sort_temp_bytes(n, 32 + node_bits((size_t)B * (size_t)N)), b = ug_scan_temp_bytes(n);
  L.temp_bytes = a > b ? a : b;
  L.temp = cv.take(L.temp_bytes);
  L.total = cv.off;
  return L;
}

// one record per (direction, sorted position): destination v (found in row_ptr), source u, fact id.  Key (v, u); a
// fact with u == v is given the key (B*N, 0): it sorts behind every node and is never a run head.
__global__ __launch_bounds__(256) void k_ug_emit(const int32_t* __restrict__ row_ptr0, const int32_t* __restrict__ row_ptr1,
                                                 const int2* __restrict__ edge0, const int2* __restrict__ edge1,
                                                 const int32_t* __restrict__ perm0, const int32_t* __restrict__ perm1,
                                                 int64_t F, int32_t BN, unsigned long long* __restrict__ keys,
                                                 int32_t* __restrict__ vals) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= 2 * F) return;
  const int d = i >= F;
  const int32_t p = (int32_t)(d ? i - F : i);
  const int32_t* rp = d ? row_ptr1 : row_ptr0;
  int lo = 0, hi = BN;                       // largest v with rp[v] <= p  (rp[0] = 0 <= p < F = rp[BN])
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (rp[mid] <= p) lo = mid; else hi = mid;
  }
  const int32_t v = lo;
  const int32_t u = (d ? edge1 : edge0)[p].x;
  const bool drop = u == v || u < 0 || u >= BN;
  keys[i] = drop ? ((unsigned long long)(unsigned)BN << 32) : (((unsigned long long)(unsigned)v << 32) | (unsigned)u);
  vals[i] = (d ? perm1 : perm0)[p];
}

__global__ __launch_bounds__(256) void k_ug_heads(const unsigned long long* __restrict__ keys, int64_t n, int32_t BN,
                                                  int32_t* __restrict__ flag) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const unsigned long long k = keys[i];
  flag[i] = (k >> 32) < (unsigned long long)(unsigned)BN && (i == 0 || keys[i - 1] != k);
}

// the head of every (v, u) run writes the pair's record: (u, largest fact id of the run)
__global__ __launch_bounds__(256) void k_ug_compact(const unsigned long long* __restrict__ keys,
                                                    const int32_t* __restrict__ facts, const int32_t* __restrict__ flag,
                                                    const int32_t* __restrict__ pos, int64_t n, int2* __restrict__ u_adj) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n || !flag[i]) return;
  const unsigned long long k = keys[i];
  int32_t best = facts[i];
  for (int64_t j = i + 1; j < n && keys[j] == k; ++j) best = max(best, facts[j]);
  u_adj[pos[i]] = make_int2((int32_t)(k & 0xffffffffu), best);
}

__global__ __launch_bounds__(256) void k_ug_ptr(const unsigned long long* __restrict__ keys,
                                                const int32_t* __restrict__ flag, const int32_t* __restrict__ pos,
                                                int64_t n, int32_t BN, int32_t* __restrict__ u_ptr) {
  const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (v > BN) return;
  const unsigned long long want = (unsigned long long)v << 32;
  int64_t lo = 0, hi = n;                    // first i with keys[i] >= want
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] < want) lo = mid + 1; else hi = mid;
  }
  u_ptr[v] = lo < n ? pos[lo] : pos[n - 1] + flag[n - 1];
}

// ---- levels and path counts ----------------------------------------------------------------------------------------------
// LDS: hdr[4] | scan[kPathThreads] | hub[kPathHubCap] | lev[N] bytes.
__global__ __launch_bounds__(kPathThreads) void k_paths_bfs(
    const int32_t* __restrict__ u_ptr, const int2* __restrict__ u_adj, int32_t N, const uint8_t* __restrict__ seed_flag,
    const int32_t* __restrict__ cand_slot, const int32_t* __restrict__ cand_cnt, int32_t S, int32_t C, int32_t max_paths,
    int32_t max_hops, uint8_t* lev_ws, unsigned* sig_ws, int32_t* __restrict__ q_info, int32_t* __restrict__ pair_info,
    int32_t* __restrict__ pair_cnt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int32_t* hdr = (int32_t*)smem;
  int32_t* scan = hdr + 4;
  int32_t* hub = scan + kPathThreads;
  uint8_t* lev = (uint8_t*)(hub + kPathHubCap);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int kWaves = kPathThreads / 64;
  const int b = blockIdx.x / S, si = blockIdx.x % S;
  const int32_t base = b * N;
  const int32_t* ptr = u_ptr + base;
  const int32_t* cs = cand_slot + (size_t)b * N;
  const int nc = min(max(cand_cnt[2 * b + 1], 0), min(C, N));
  const size_t pair0 = ((size_t)b * S + si) * C;
  uint8_t* levw = lev_ws + ((size_t)b * S + si) * N;
  unsigned* sig = sig_ws + ((size_t)b * S + si) * N;

  // the si-th seed of the question (ascending slot) and the number of seeds: counts of contiguous chunks, scanned
  const int chunk = (N + kPathThreads - 1) / kPathThreads;
  const int c0 = min(tid * chunk, N), c1 = min(c0 + chunk, N);
  const uint8_t* sf = seed_flag + (size_t)b * N;
  int mine = 0;
  for (int v = c0; v < c1; ++v) mine += sf[v] != 0;
  scan[tid] = mine;
  if (tid == 0) hdr[2] = -1;
  __syncthreads();
  for (int d = 1; d < kPathThreads; d <<= 1) {
    const int add = tid >= d ? scan[tid - d] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  {
    int before = scan[tid] - mine;
    if (si >= before && si < before + mine)
      for (int v = c0; v < c1; ++v)
        if (sf[v] != 0 && before++ == si) hdr[2] = v;
  }
  const int n_seeds = scan[kPathThreads - 1];
  __syncthreads();
  const int s = hdr[2];
  if (si == 0 && tid == 0) {
    q_info[2 * b] = n_seeds;
    q_info[2 * b + 1] = max(cand_cnt[2 * b + 1], 0);
  }
  if (s < 0) {                               // fewer than si + 1 seeds: empty pairs
    for (int t = tid; t < C; t += kPathThreads) {
      pair_info[2 * (pair0 + t)] = 0;
      pair_info[2 * (pair0 + t) + 1] = -1;
      pair_cnt[pair0 + t] = 0;
    }
    return;
  }

  // rows a wave scans: ascending list, built from per-wave counts of contiguous node ranges (no atomics)
  for (int v = tid; v < N; v += kPathThreads) lev[v] = (uint8_t)kUnvisited;
  const int wchunk = ((N + kWaves - 1) / kWaves + 63) / 64 * 64;
  const int w0 = min(wave * wchunk, N), w1 = min(w0 + wchunk, N);
  int wcnt = 0;
  for (int v0 = w0; v0 < w1; v0 += 64) {
    const int v = v0 + lane;
    const bool heavy = v < w1 && ptr[v + 1] - ptr[v] > kPathLaneDeg;
    wcnt += __popcll(__ballot(heavy));
  }
  __syncthreads();                           // scan[] is free again
  if (lane == 0) scan[wave] = wcnt;
  __syncthreads();
  int wpos = 0, n_hub = 0;
  for (int w = 0; w < kWaves; ++w) {
    if (w < wave) wpos += scan[w];
    n_hub += scan[w];
  }
  for (int v0 = w0; v0 < w1; v0 += 64) {
    const int v = v0 + lane;
    const bool heavy = v < w1 && ptr[v + 1] - ptr[v] > kPathLaneDeg;
    const unsigned long long m = __ballot(heavy);
    if (heavy) {
      const int at = wpos + __popcll(m & ((1ull << lane) - 1ull));
      if (at < kPathHubCap) hub[at] = v;
    }
    wpos += __popcll(m);
  }
  if (tid == 0) {
    lev[s] = 0;
    sig[s] = 1u;
  }
  __syncthreads();
  const int n_list = min(n_hub, kPathHubCap);
  const int hub_last = n_hub > kPathHubCap ? hub[kPathHubCap - 1] : N;      // rows <= hub_last with many neighbours: a wave

  int l = 0;
  while (true) {
    int open = 0;
    for (int t = tid; t < nc; t += kPathThreads) {
      const int c = cs[t];
      open |= c >= 0 && c < N && lev[c] == kUnvisited;
    }
    if (!block_or(open, hdr + 3)) break;     // every candidate has its level (and its complete count)
    if (l >= max_hops) break;
    ++l;
    const unsigned prev = (unsigned)(l - 1);
    int found = 0;
    // a node written in this round holds l or "not reached", never l - 1: no atomics, one barrier per level
    for (int v = tid; v < N; v += kPathThreads) {
      if (lev[v] != kUnvisited) continue;
      const int e0 = ptr[v], e1 = ptr[v + 1];
      if (e1 - e0 > kPathLaneDeg && v <= hub_last) continue;
      unsigned acc = 0;
      bool any = false;
      for (int e = e0; e < e1; ++e) {
        const unsigned u = (unsigned)(u_adj[e].x - base);
        if (u < (unsigned)N && lev[u] == prev) {
          acc = sat_add(acc, sig[u]);
          any = true;
        }
      }
      if (any) {
        lev[v] = (uint8_t)l;
        sig[v] = acc;
        found = 1;
      }
    }
    for (int h = wave; h < n_list; h += kWaves) {
      const int v = hub[h];
      if (lev[v] != kUnvisited) continue;
      const int e0 = ptr[v], e1 = ptr[v + 1];
      unsigned acc = 0;
      int any = 0;
      for (int e = e0 + lane; e < e1; e += 64) {
        const unsigned u = (unsigned)(u_adj[e].x - base);
        if (u < (unsigned)N && lev[u] == prev) {
          acc = sat_add(acc, sig[u]);
          any = 1;
        }
      }
      for (int o = 32; o > 0; o >>= 1) {
        acc = sat_add(acc, (unsigned)__shfl_xor((int)acc, o));
        any |= __shfl_xor(any, o);
      }
      if (any && lane == 0) {
        lev[v] = (uint8_t)l;
        sig[v] = acc;
      }
      found |= any;
    }
    if (!block_or(found, hdr + 3)) break;    // the component is exhausted
  }
  __syncthreads();
  for (int v = tid; v < N; v += kPathThreads) levw[v] = lev[v];
  const bool seed_has_edge = ptr[s + 1] > ptr[s];
  for (int t = tid; t < C; t += kPathThreads) {
    int n = 0, h = -1;
    if (t < nc && seed_has_edge) {
      const int c = cs[t];
      if (c >= 0 && c < N && lev[c] != kUnvisited) {
        n = (int)sig[c];
        h = lev[c];
      }
    }
    pair_info[2 * (pair0 + t)] = n;
    pair_info[2 * (pair0 + t) + 1] = h;
    pair_cnt[pair0 + t] = min(n, max_paths);
  }
}

// off[0 .. P] = exclusive scan of cnt(0 .. P-1); one workgroup, contiguous chunk per thread
template <class Cnt>
__device__ __forceinline__ void paths_offsets_body(Cnt cnt, int64_t P, int32_t* __restrict__ off) {
  __shared__ int32_t part[1024];
  const int tid = threadIdx.x;
  const int64_t chunk = (P + 1023) / 1024;
  const int64_t p0 = min((int64_t)tid * chunk, P), p1 = min(p0 + chunk, P);
  int32_t mine = 0;
  for (int64_t p = p0; p < p1; ++p) mine += cnt(p);
  part[tid] = mine;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int32_t add = tid >= d ? part[tid - d] : 0;
    __syncthreads();
    part[tid] += add;
    __syncthreads();
  }
  int32_t run = part[tid] - mine;
  for (int64_t p = p0; p < p1; ++p) {
    off[p] = run;
    run += cnt(p);
  }
  if (tid == 1023) off[P] = part[1023];
}

__global__ __launch_bounds__(1024) void k_paths_offsets(const int32_t* __restrict__ cnt, int64_t P,
                                                        int32_t* __restrict__ off) {
  paths_offsets_body([cnt](int64_t p) { return cnt[p]; }, P, off);
}

// one wave per pair, one lane per written path: rank k -> the k-th path in the order "node sequence read from the
// candidate back to the seed, ascending node id".  Records are written compactly at off[pair] + k.
__global__ __launch_bounds__(64) void k_paths_unrank(const int32_t* __restrict__ u_ptr, const int2* __restrict__ u_adj,
                                                     int32_t N, const int32_t* __restrict__ cand_slot, int32_t S, int32_t C,
                                                     int32_t max_hops, const uint8_t* __restrict__ lev_ws,
                                                     const unsigned* __restrict__ sig_ws,
                                                     const int32_t* __restrict__ pair_info, const int32_t* __restrict__ off,
                                                     int32_t* __restrict__ path_nodes, int32_t* __restrict__ path_facts) {
  const size_t p = blockIdx.x;
  const int32_t o0 = off[p], n = off[p + 1] - o0;
  if (n <= 0) return;
  const int t = (int)(p % C);
  const size_t bs = p / C;
  const int b = (int)(bs / S);
  const int32_t base = b * N;
  const int32_t* ptr = u_ptr + base;
  const uint8_t* lev = lev_ws + bs * N;
  const unsigned* sig = sig_ws + bs * N;
  const int c = cand_slot[(size_t)b * N + t];
  const int hops = pair_info[2 * p + 1];
  for (int k = threadIdx.x; k < n; k += 64) {
    int32_t* nodes = path_nodes + ((size_t)o0 + k) * (size_t)(max_hops + 1);
    int32_t* facts = path_facts + ((size_t)o0 + k) * (size_t)max_hops;
    for (int i = hops + 1; i <= max_hops; ++i) nodes[i] = -1;
    for (int i = hops; i < max_hops; ++i) facts[i] = -1;
    nodes[hops] = base + c;
    unsigned r = (unsigned)k;
    int v = c, step = hops;
    for (; step > 0; --step) {
      const int e0 = ptr[v], e1 = ptr[v + 1];
      int pick = -1, fact = -1;
      for (int e = e0; e < e1; ++e) {
        const int2 a = u_adj[e];
        const unsigned u = (unsigned)(a.x - base);
        if (u < (unsigned)N && lev[u] == (unsigned)(step - 1)) {
          const unsigned sg = sig[u];
          if (r < sg) {
            pick = (int)u;
            fact = a.y;
            break;
          }
          r -= sg;
        }
      }
      if (pick < 0) break;                   // cannot happen for counts made by k_paths_bfs
      nodes[step - 1] = base + pick;
      facts[step - 1] = fact;
      v = pick;
    }
    for (; step > 0; --step) {
      nodes[step - 1] = -1;
      facts[step - 1] = -1;
    }
  }
}

struct PathWs {
  size_t cnt, lev, sig, total;
};

static PathWs path_ws_layout(int32_t B, int32_t N, int32_t S, int32_t C) {
  PathWs L;
  Carve cv;
  L.cnt = cv.take((size_t)B * S * C * 4);
  L.lev = cv.take((size_t)B * S * N);
  L.sig = cv.take((size_t)B * S * N * 4);
  L.total = cv.off;
  return L;
}

static bool path_limits_ok(int32_t B, int32_t S, int32_t C) { return B > 0 && S > 0 && C > 0; }

// ---- rule-guided walks -------------------------------------------------------------------------------------------------
// bfs_with_rule(G, start, rule) returns every walk start = v0 .. vL whose hop i is an edge of relation rule[i] (nodes and
// edges may repeat).  The number of walks from v that complete the rule from hop l on does not depend on the seed:
//   down_L = 1,   down_l[v] = sum over neighbours u of v with rel(v, u) == rule[l] of down_{l+1}[u]
// so the counts are made once per (question, rule) and every seed of the question reads n_paths = down_0[seed].
//
// Workspace: erel [2 max(F, 1)] int32 | down [B][max_rules][max_hops][N] uint32 (level L is not stored), each rounded up
// to 256 bytes.  The relation of an adjacency record is staged once per call (erel[e] = fact_rel[u_adj[e].y]) rather than
// gathered per use: every (rule, level) of a question scans the question's records again, a stream beside u_adj instead
// of a dependent random read.  kRuleNoRel marks a record whose fact id is out of range; it matches no rule.
constexpr int kRuleThreads = 512;          // k_rule_counts: 8 waves per (question, rule)
constexpr int kRuleSeedThreads = 256;      // k_rule_unrank: 4 waves per (question, seed)
constexpr int32_t kRuleNoRel = INT32_MIN;

struct RuleWs {
  size_t erel, down, total;
};

static bool rule_sizes_ok(int64_t F, int32_t B, int32_t N, int32_t R, int32_t H) {
  return F >= 0 && 2 * F < INT32_MAX && B > 0 && N > 0 && R > 0 && H > 0 && (int64_t)B * N < INT32_MAX &&
         (int64_t)B * R < INT32_MAX;
}

static RuleWs rule_ws_layout(int64_t F, int32_t B, int32_t N, int32_t R, int32_t H) {     // H <= 254, N <= 65536: no wrap
  RuleWs L;
  L.erel = 0;
  L.down = align_up(2 * (size_t)(F > 0 ? F : 1) * 4, 256);
  L.total = L.down + align_up((size_t)B * R * H * N * 4, 256);
  return L;
}

__global__ __launch_bounds__(256) void k_rule_edge_rel(const int32_t* __restrict__ u_ptr, const int2* __restrict__ u_adj,
                                                       int32_t BN, int64_t cap, int64_t F,
                                                       const int32_t* __restrict__ fact_rel, int32_t* __restrict__ erel) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= cap || e >= u_ptr[BN]) return;
  const int32_t f = u_adj[e].y;
  erel[e] = f >= 0 && f < F ? fact_rel[f] : kRuleNoRel;
}

// si-th set byte of flag[0 .. N) in ascending order (-1: there are fewer) and the number of set bytes; whole workgroup of
// T threads, scan = T ints of LDS, hit = one int of LDS.  Counts of contiguous chunks, scanned: no atomics.
template <int T>
__device__ __forceinline__ int nth_seed(const uint8_t* __restrict__ flag, int N, int si, int32_t* scan, int32_t* hit,
                                        int* n_seeds) {
  const int tid = threadIdx.x;
  const int chunk = (N + T - 1) / T;
  const int c0 = min(tid * chunk, N), c1 = min(c0 + chunk, N);
  int mine = 0;
  for (int v = c0; v < c1; ++v) mine += flag[v] != 0;
  scan[tid] = mine;
  if (tid == 0) *hit = -1;
  __syncthreads();
  for (int d = 1; d < T; d <<= 1) {
    const int add = tid >= d ? scan[tid - d] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  int before = scan[tid] - mine;
  if (si >= before && si < before + mine)
    for (int v = c0; v < c1; ++v)
      if (flag[v] != 0 && before++ == si) *hit = v;
  *n_seeds = scan[T - 1];
  __syncthreads();
  return *hit;
}

// one workgroup per (question, rule).  Rows of at most kPathLaneDeg records: a lane each; heavier rows (the first
// kPathHubCap of the question, ascending) are listed once and summed by a wave, as in k_paths_bfs.  A level reads only
// the level above it, written before the barrier: one barrier per level.
__global__ __launch_bounds__(kRuleThreads) void k_rule_counts(
    const int32_t* __restrict__ u_ptr, const int2* __restrict__ u_adj, const int32_t* __restrict__ erel, int64_t cap,
    int32_t N, const uint8_t* __restrict__ seed_flag, const int32_t* __restrict__ rule_rel,
    const int32_t* __restrict__ rule_len, int32_t S, int32_t R, int32_t H, unsigned* down_ws, int32_t* __restrict__ q_info,
    int32_t* __restrict__ pair_info) {
  __shared__ int32_t scan[kRuleThreads];
  __shared__ int32_t hub[kPathHubCap];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int kWaves = kRuleThreads / 64;
  const int b = blockIdx.x / R, k = blockIdx.x % R;
  const int32_t base = b * N;
  const int32_t* ptr = u_ptr + base;
  const int32_t* rule = rule_rel + ((size_t)b * R + k) * H;
  const int L = rule_len[(size_t)b * R + k];
  const bool valid = L >= 1 && L <= H;
  unsigned* down = down_ws + ((size_t)b * R + k) * H * (size_t)N;

  if (valid) {
    // rows a wave scans: ascending list, built from per-wave counts of contiguous node ranges
    const int wchunk = ((N + kWaves - 1) / kWaves + 63) / 64 * 64;
    const int w0 = min(wave * wchunk, N), w1 = min(w0 + wchunk, N);
    int wcnt = 0;
    for (int v0 = w0; v0 < w1; v0 += 64) {
      const int v = v0 + lane;
      const bool heavy = v < w1 && ptr[v + 1] - ptr[v] > kPathLaneDeg;
      wcnt += __popcll(__ballot(heavy));
    }
    if (lane == 0) scan[wave] = wcnt;
    __syncthreads();
    int wpos = 0, n_hub = 0;
    for (int w = 0; w < kWaves; ++w) {
      if (w < wave) wpos += scan[w];
      n_hub += scan[w];
    }
    for (int v0 = w0; v0 < w1; v0 += 64) {
      const int v = v0 + lane;
      const bool heavy = v < w1 && ptr[v + 1] - ptr[v] > kPathLaneDeg;
      const unsigned long long m = __ballot(heavy);
      if (heavy) {
        const int at = wpos + __popcll(m & ((1ull << lane) - 1ull));
        if (at < kPathHubCap) hub[at] = v;
      }
      wpos += __popcll(m);
    }
    __syncthreads();
    const int n_list = min(n_hub, kPathHubCap);
    const int hub_last = n_hub > kPathHubCap ? hub[kPathHubCap - 1] : N;

    for (int l = L - 1; l >= 0; --l) {
      const int32_t want = rule[l];
      const bool dead = want == kRuleNoRel;
      const bool last = l == L - 1;
      const unsigned* nxt = down + (size_t)(last ? l : l + 1) * N;       // not read when last
      unsigned* cur = down + (size_t)l * N;
      for (int v = tid; v < N; v += kRuleThreads) {
        const int64_t e0 = min((int64_t)max(ptr[v], 0), cap), e1 = min((int64_t)max(ptr[v + 1], 0), cap);
        if (e1 - e0 > kPathLaneDeg && v <= hub_last) continue;
        unsigned acc = 0;
        if (!dead)
          for (int64_t e = e0; e < e1; ++e) {
            if (erel[e] != want) continue;
            const unsigned u = (unsigned)(u_adj[e].x - base);
            if (u < (unsigned)N) acc = sat_add(acc, last ? 1u : nxt[u]);
          }
        cur[v] = acc;
      }
      for (int h = wave; h < n_list; h += kWaves) {
        const int v = hub[h];
        const int64_t e0 = min((int64_t)max(ptr[v], 0), cap), e1 = min((int64_t)max(ptr[v + 1], 0), cap);
        unsigned acc = 0;
        if (!dead)
          for (int64_t e = e0 + lane; e < e1; e += 64) {
            if (erel[e] != want) continue;
            const unsigned u = (unsigned)(u_adj[e].x - base);
            if (u < (unsigned)N) acc = sat_add(acc, last ? 1u : nxt[u]);
          }
        for (int o = 32; o > 0; o >>= 1) acc = sat_add(acc, (unsigned)__shfl_xor((int)acc, o));
        if (lane == 0) cur[v] = acc;
      }
      __syncthreads();
    }
  }

  // the question's seeds in ascending order: seed index i reads down_0 of its slot
  const uint8_t* sf = seed_flag + (size_t)b * N;
  const int chunk = (N + kRuleThreads - 1) / kRuleThreads;
  const int c0 = min(tid * chunk, N), c1 = min(c0 + chunk, N);
  int mine = 0;
  for (int v = c0; v < c1; ++v) mine += sf[v] != 0;
  __syncthreads();                           // scan[] is free again
  scan[tid] = mine;
  __syncthreads();
  for (int d = 1; d < kRuleThreads; d <<= 1) {
    const int add = tid >= d ? scan[tid - d] : 0;
    __syncthreads();
    scan[tid] += add;
    __syncthreads();
  }
  const int n_seeds = scan[kRuleThreads - 1];
  int idx = scan[tid] - mine;
  for (int v = c0; v < c1 && idx < S; ++v) {
    if (sf[v] == 0) continue;
    const size_t p = ((size_t)b * S + idx) * R + k;
    pair_info[2 * p] = valid ? (int32_t)down[v] : 0;
    pair_info[2 * p + 1] = valid ? L : -1;
    ++idx;
  }
  for (int i = max(n_seeds, 0) + tid; i < S; i += kRuleThreads) {         // fewer than i + 1 seeds: empty pairs
    const size_t p = ((size_t)b * S + i) * R + k;
    pair_info[2 * p] = 0;
    pair_info[2 * p + 1] = -1;
  }
  if (k == 0) {
    int ok = 0;
    for (int i = tid; i < R; i += kRuleThreads) {
      const int len = rule_len[(size_t)b * R + i];
      ok += len >= 1 && len <= H;
    }
    __syncthreads();
    scan[tid] = ok;
    __syncthreads();
    for (int d = kRuleThreads / 2; d > 0; d >>= 1) {
      if (tid < d) scan[tid] += scan[tid + d];
      __syncthreads();
    }
    if (tid == 0) {
      q_info[2 * b] = n_seeds;
      q_info[2 * b + 1] = scan[0];
    }
  }
}

__global__ __launch_bounds__(1024) void k_rule_offsets(const int32_t* __restrict__ pair_info, int32_t max_paths, int64_t P,
                                                       int32_t* __restrict__ off) {
  paths_offsets_body([=](int64_t p) { return min(max(pair_info[2 * p], 0), max_paths); }, P, off);
}

// one workgroup per (question, seed index), one lane per written record: rank k -> the k-th walk in the order "node
// sequence read from the seed outwards, ascending node id".  At hop l the matching neighbours u of the current node are
// passed in ascending order, each standing for down_{l+1}[u] walks.  A saturated count is only ever compared with a rank
// below max_paths <= INT32_MAX, so it stops the scan where the true count would.
__global__ __launch_bounds__(kRuleSeedThreads) void k_rule_unrank(
    const int32_t* __restrict__ u_ptr, const int2* __restrict__ u_adj, const int32_t* __restrict__ erel, int64_t cap,
    int32_t N, const uint8_t* __restrict__ seed_flag, const int32_t* __restrict__ rule_rel, int32_t S, int32_t R, int32_t H,
    const unsigned* __restrict__ down_ws, const int32_t* __restrict__ pair_info, const int32_t* __restrict__ off,
    int64_t n_rec, int32_t* __restrict__ path_nodes, int32_t* __restrict__ path_facts) {
  __shared__ int32_t scan[kRuleSeedThreads];
  __shared__ int32_t hit;
  const int b = blockIdx.x / S, si = blockIdx.x % S;
  const size_t pair0 = (size_t)blockIdx.x * R;
  if (off[pair0 + R] == off[pair0]) return;  // nothing to write for this seed (uniform over the workgroup)
  int n_seeds;
  const int s = nth_seed<kRuleSeedThreads>(seed_flag + (size_t)b * N, N, si, scan, &hit, &n_seeds);
  if (s < 0) return;
  const int32_t base = b * N;
  const int32_t* ptr = u_ptr + base;
  for (int r = 0; r < R; ++r) {
    const size_t p = pair0 + r;
    const int64_t o0 = off[p];
    const int n = (int)(off[p + 1] - o0);
    const int L = pair_info[2 * p + 1];
    if (n <= 0 || L < 1 || L > H || o0 < 0 || o0 + n > n_rec) continue;
    const int32_t* rule = rule_rel + ((size_t)b * R + r) * H;
    const unsigned* down = down_ws + ((size_t)b * R + r) * H * (size_t)N;
    for (int k = threadIdx.x; k < n; k += kRuleSeedThreads) {
      int32_t* nodes = path_nodes + (size_t)(o0 + k) * (size_t)(H + 1);
      int32_t* facts = path_facts + (size_t)(o0 + k) * (size_t)H;
      nodes[0] = base + s;
      unsigned rank = (unsigned)k;
      int v = s, l = 0;
      for (; l < L; ++l) {
        const int32_t want = rule[l];
        const bool last = l == L - 1;
        const unsigned* nxt = down + (size_t)(last ? l : l + 1) * N;
        const int64_t e0 = min((int64_t)max(ptr[v], 0), cap), e1 = min((int64_t)max(ptr[v + 1], 0), cap);
        int pick = -1, fact = -1;
        if (want != kRuleNoRel)
          for (int64_t e = e0; e < e1; ++e) {
            if (erel[e] != want) continue;
            const int2 a = u_adj[e];
            const unsigned u = (unsigned)(a.x - base);
            if (u >= (unsigned)N) continue;
            const unsigned d = last ? 1u : nxt[u];
            if (rank < d) {
              pick = (int)u;
              fact = a.y;
              break;
            }
            rank -= d;
          }
        if (pick < 0) break;                 // cannot happen for counts made by k_rule_counts
        nodes[l + 1] = base + pick;
        facts[l] = fact;
        v = pick;
      }
      for (int i = l; i < H; ++i) {
        nodes[i + 1] = -1;
        facts[i] = -1;
      }
    }
  }
}

}  // namespace gnnrag

using namespace gnnrag;

extern "C" size_t gnnrag_ugraph_bytes(int64_t F, int32_t B, int32_t N) {
  if (F < 0 || B <= 0 || N <= 0 || (int64_t)B * N >= INT32_MAX || 2 * F >= INT32_MAX) return 0;
  return align_up(((size_t)B * N + 1) * 4, 256) + align_up(2 * (size_t)(F > 0 ? F : 1) * 8, 256);
}

extern "C" size_t gnnrag_ugraph_scratch_bytes(int64_t F, int32_t B, int32_t N) {
  if (F < 0 || B <= 0 || N <= 0 || (int64_t)B * N >= INT32_MAX || 2 * F >= INT32_MAX) return 0;
  return ug_scratch_layout(F, B, N).total;
}

extern "C" int gnnrag_ugraph_build(const gnnrag_csr* csr, void* mem, size_t mem_bytes, void* scratch, size_t scratch_bytes,
                                   gnnrag_ugraph* out, gnnrag_stream_t stream_) {
  if (!csr || !mem || !scratch || !out) return GNNRAG_E_BADARG;
  const int64_t F = csr->F;
  const int32_t B = csr->B, N = csr->N;
  if (F < 0 || B <= 0 || N <= 0 || (int64_t)B * N >= INT32_MAX || 2 * F >= INT32_MAX) return GNNRAG_E_BADARG;
  for (int d = 0; d < 2; ++d)
    if (!csr->row_ptr[d] || (F > 0 && (!csr->edge[d] || !csr->perm[d]))) return GNNRAG_E_BADARG;
  if (mem_bytes < gnnrag_ugraph_bytes(F, B, N)) return GNNRAG_E_WORKSPACE;
  const UgScratch L = ug_scratch_layout(F, B, N);
  if (scratch_bytes < L.total) return GNNRAG_E_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  const int32_t BN = B * N;
  out->B = B;
  out->N = N;
  out->F = F;
  out->cap = 2 * (F > 0 ? F : 1);
  out->u_ptr = (int32_t*)mem;
  out->u_adj = (int32_t*)((char*)mem + align_up(((size_t)BN + 1) * 4, 256));
  if (F == 0) {
    GNNRAG_HIP(hipMemsetAsync(out->u_ptr, 0, ((size_t)BN + 1) * 4, stream));
    return 0;
  }
  char* sc = (char*)scratch;
  unsigned long long* key_in = (unsigned long long*)(sc + L.key_in);
  unsigned long long* key_out = (unsigned long long*)(sc + L.key_out);
  int32_t* val_in = (int32_t*)(sc + L.val_in);
  int32_t* val_out = (int32_t*)(sc + L.val_out);
  int32_t* flag = (int32_t*)(sc + L.flag);
  int32_t* pos = (int32_t*)(sc + L.scan);
  const int64_t n = 2 * F;
  const unsigned grid = (unsigned)((n + 255) / 256);
  k_ug_emit<<<grid, 256, 0, stream>>>(csr->row_ptr[0], csr->row_ptr[1], (const int2*)csr->edge[0],
                                      (const int2*)csr->edge[1], csr->perm[0], csr->perm[1], F, BN, key_in, val_in);
  GNNRAG_LAUNCH_CHECK();
  size_t tb = L.temp_bytes;
  GNNRAG_HIP(rocprim::radix_sort_pairs(sc + L.temp, tb, (const unsigned long long*)key_in, key_out,
                                       (const int32_t*)val_in, val_out, (size_t)n, 0u, 32 + node_bits((size_t)BN), stream,
                                       false));
  k_ug_heads<<<grid, 256, 0, stream>>>(key_out, n, BN, flag);
  GNNRAG_LAUNCH_CHECK();
  tb = L.temp_bytes;
  GNNRAG_HIP(rocprim::exclusive_scan(sc + L.temp, tb, (const int32_t*)flag, pos, (int32_t)0, (size_t)n,
                                     rocprim::plus<int32_t>(), stream, false));
  k_ug_compact<<<grid, 256, 0, stream>>>(key_out, val_out, flag, pos, n, (int2*)out->u_adj);
  GNNRAG_LAUNCH_CHECK();
  k_ug_ptr<<<(unsigned)(((int64_t)BN + 1 + 255) / 256), 256, 0, stream>>>(key_out, flag, pos, n, BN, out->u_ptr);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t gnnrag_paths_workspace_bytes(int32_t B, int32_t N, int32_t max_seeds, int32_t max_cands) {
  if (!path_limits_ok(B, max_seeds, max_cands) || N <= 0 || N > kPathMaxN) return 0;
  if ((int64_t)B * max_seeds * max_cands >= INT32_MAX) return 0;
  return path_ws_layout(B, N, max_seeds, max_cands).total;
}

extern "C" size_t gnnrag_paths_out_bytes(int32_t B, int32_t max_seeds, int32_t max_cands, int32_t max_paths,
                                         int32_t max_hops) {
  if (!path_limits_ok(B, max_seeds, max_cands) || max_paths <= 0 || max_hops <= 0 || max_hops > kPathMaxHops) return 0;
  const int64_t P = (int64_t)B * max_seeds * max_cands;
  if (P >= INT32_MAX || P * max_paths >= INT32_MAX) return 0;
  const size_t rec = (size_t)P * max_paths;
  return align_up((size_t)B * 8, 256) + align_up((size_t)P * 8, 256) + align_up(((size_t)P + 1) * 4, 256) +
         align_up(rec * (size_t)(max_hops + 1) * 4, 256) + align_up(rec * (size_t)max_hops * 4, 256);
}

extern "C" int gnnrag_shortest_paths(const gnnrag_ugraph* g, const uint8_t* seed_flag, const int32_t* cand_slot,
                                     const int32_t* cand_cnt, int32_t max_seeds, int32_t max_cands, int32_t max_paths,
                                     int32_t max_hops, int32_t* q_info, int32_t* pair_info, int32_t* path_off,
                                     int32_t* path_nodes, int32_t* path_facts, void* workspace, size_t workspace_bytes,
                                     gnnrag_stream_t stream_) {
  if (!g || !seed_flag || !cand_slot || !cand_cnt || !q_info || !pair_info || !path_off || !path_nodes || !path_facts ||
      !workspace)
    return GNNRAG_E_BADARG;
  if (g->B <= 0 || g->N <= 0 || !g->u_ptr || !g->u_adj || max_seeds <= 0 || max_cands <= 0 || max_paths <= 0 ||
      max_hops <= 0)
    return GNNRAG_E_BADARG;
  if (max_hops > kPathMaxHops || g->N > kPathMaxN) return GNNRAG_E_UNSUPPORTED;
  const int32_t B = g->B, N = g->N, S = max_seeds, C = max_cands;
  const int64_t P = (int64_t)B * S * C;
  if (P >= INT32_MAX || P * max_paths >= INT32_MAX || (int64_t)B * S > 0x7fffffff) return GNNRAG_E_UNSUPPORTED;
  const PathWs L = path_ws_layout(B, N, S, C);
  if (workspace_bytes < L.total) return GNNRAG_E_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  int32_t* cnt = (int32_t*)(ws + L.cnt);
  uint8_t* lev = (uint8_t*)(ws + L.lev);
  unsigned* sig = (unsigned*)(ws + L.sig);
  static DeviceMask lds_done{0};
  GNNRAG_RC(raise_lds_cap(k_paths_bfs, lds_done));
  const size_t lds = align_up(kPathLdsFixed + (size_t)N, 16);
  k_paths_bfs<<<(unsigned)(B * S), kPathThreads, lds, stream>>>(g->u_ptr, (const int2*)g->u_adj, N, seed_flag, cand_slot,
                                                                cand_cnt, S, C, max_paths, max_hops, lev, sig, q_info,
                                                                pair_info, cnt);
  GNNRAG_LAUNCH_CHECK();
  k_paths_offsets<<<1, 1024, 0, stream>>>(cnt, P, path_off);
  GNNRAG_LAUNCH_CHECK();
  k_paths_unrank<<<(unsigned)P, 64, 0, stream>>>(g->u_ptr, (const int2*)g->u_adj, N, cand_slot, S, C, max_hops, lev, sig,
                                                 pair_info, path_off, path_nodes, path_facts);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}

extern "C" size_t gnnrag_rule_paths_workspace_bytes(int64_t F, int32_t B, int32_t N, int32_t max_rules, int32_t max_hops) {
  if (!rule_sizes_ok(F, B, N, max_rules, max_hops) || max_hops > kPathMaxHops || N > kPathMaxN) return 0;
  return rule_ws_layout(F, B, N, max_rules, max_hops).total;
}

extern "C" size_t gnnrag_rule_paths_out_bytes(int32_t B, int32_t max_seeds, int32_t max_rules, int32_t max_paths,
                                              int32_t max_hops) {
  return gnnrag_paths_out_bytes(B, max_seeds, max_rules, max_paths, max_hops);      // the same five arrays, C = max_rules
}

extern "C" int gnnrag_rule_paths(const gnnrag_ugraph* g, const int32_t* fact_rel, const uint8_t* seed_flag,
                                 const int32_t* rule_rel, const int32_t* rule_len, int32_t max_seeds, int32_t max_rules,
                                 int32_t max_paths, int32_t max_hops, int32_t* q_info, int32_t* pair_info,
                                 int32_t* path_off, int32_t* path_nodes, int32_t* path_facts, void* workspace,
                                 size_t workspace_bytes, gnnrag_stream_t stream_) {
  if (!g || !seed_flag || !rule_rel || !rule_len || !q_info || !pair_info || !path_off || !path_nodes || !path_facts ||
      !workspace)
    return GNNRAG_E_BADARG;
  if (g->B <= 0 || g->N <= 0 || g->F < 0 || !g->u_ptr || !g->u_adj || (g->F > 0 && !fact_rel) || max_seeds <= 0 ||
      max_rules <= 0 || max_paths <= 0 || max_hops <= 0)
    return GNNRAG_E_BADARG;
  const int32_t B = g->B, N = g->N, S = max_seeds, R = max_rules, H = max_hops;
  const int64_t F = g->F;
  if (H > kPathMaxHops || N > kPathMaxN) return GNNRAG_E_UNSUPPORTED;
  if (!rule_sizes_ok(F, B, N, R, H) || g->cap < 0 || g->cap > 2 * (F > 0 ? F : 1)) return GNNRAG_E_BADARG;
  const int64_t P = (int64_t)B * S * R;
  if (P >= INT32_MAX || P * max_paths >= INT32_MAX) return GNNRAG_E_UNSUPPORTED;
  const RuleWs L = rule_ws_layout(F, B, N, R, H);
  if (workspace_bytes < L.total) return GNNRAG_E_WORKSPACE;
  hipStream_t stream = (hipStream_t)stream_;
  char* ws = (char*)workspace;
  int32_t* erel = (int32_t*)(ws + L.erel);
  unsigned* down = (unsigned*)(ws + L.down);
  const int2* adj = (const int2*)g->u_adj;
  if (F > 0) {
    k_rule_edge_rel<<<(unsigned)((g->cap + 255) / 256), 256, 0, stream>>>(g->u_ptr, adj, B * N, g->cap, F, fact_rel, erel);
    GNNRAG_LAUNCH_CHECK();
  }
  k_rule_counts<<<(unsigned)(B * R), kRuleThreads, 0, stream>>>(g->u_ptr, adj, erel, g->cap, N, seed_flag, rule_rel,
                                                                rule_len, S, R, H, down, q_info, pair_info);
  GNNRAG_LAUNCH_CHECK();
  k_rule_offsets<<<1, 1024, 0, stream>>>(pair_info, max_paths, P, path_off);
  GNNRAG_LAUNCH_CHECK();
  k_rule_unrank<<<(unsigned)(B * S), kRuleSeedThreads, 0, stream>>>(g->u_ptr, adj, erel, g->cap, N, seed_flag, rule_rel, S,
                                                                    R, H, down, pair_info, path_off, P * max_paths,
                                                                    path_nodes, path_facts);
  GNNRAG_LAUNCH_CHECK();
  return 0;
}
