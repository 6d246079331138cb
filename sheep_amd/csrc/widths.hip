// widths.hip — the true bag sizes of an elimination tree: width(v) = 1 + |jxn(v)|, where
// jxn(v) is the set of later vertices adjacent to v's subtree (jtree.cpp:97 newUnion,
// jnode.h:230-260).  The reference materialises every junction set (under a 1 GB cap,
// jtree.h:89); only the sizes are needed here, and those are the column counts of the
// symbolic Cholesky factor.
//
// Row-subtree identity.  For a vertex u, the nodes v < u with u in jxn(v) are exactly the
// nodes on the tree paths from u's lower neighbours up to (excluding) u.  With the lower
// neighbours p_1 .. p_k in tour order, the weights
//     +1 at every p_i,  -1 at lca(p_i, p_{i+1}),  -1 at u
// sum to 1 over the subtree of every such v and to 0 over every other subtree, so
// |jxn(v)| is the sum of all weights in v's subtree: one prefix sum in tour order.
//
// Passes (no host round trip between them; every pass is a TimedRegion):
//   widths_tour     kid table + Euler tour (tree_tour.hip), subtree intervals per node
//   widths_sort     key = hi << bits(A) | tD[lo] per record (dropped records carry hi = n and
//                   sort to the end), u64 radix sort over the significant bits only
//   widths_lca      sparse table over the tour's node sequence.  A parent is always later than
//                   its kids (build_kids checks it), so the shallowest node of a tour range is
//                   its LARGEST id: the range-minimum over depths is a range-maximum over ids,
//                   and no depth array is built.  A * ceil(log2 A) * 4 bytes, A = 2 (n - roots).
//   widths_weights  one pass over the sorted keys (run_add: a hub's -1s leave a wave combined)
//   widths_sums     prefix sum in tour order, width[v] = 1 + E[tU[v]] - E[tD[v]]
#include "tree_tour.hpp"

namespace sheep {
namespace {

// flags[0]: a neighbour >= pos_size of a sequenced vertex (index.at throws, jtree.cpp:75)
// flags[1]: an edge whose lo is not a descendant of its hi (not the tree of these records)
constexpr int W_FLAGS = 2;

__global__ __launch_bounds__(BLOCK) void k_w_keys(const sheep_xs1 *__restrict__ rec, uint64_t nrec,
                                                  const uint32_t *__restrict__ pos, uint64_t pos_size,
                                                  const uint32_t *__restrict__ tD, uint64_t n, int sh,
                                                  uint64_t *__restrict__ keys, unsigned long long *__restrict__ flags) {
  // the relabel's outcomes (etree.hip k_relabel): self-loops and records with an unsequenced
  // end carry no edge
  const uint64_t stride = (uint64_t)gridDim.x * BLOCK, dead = (uint64_t)n << sh;
  bool oor = false, stray = false;
  for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < nrec; i += stride) {
    const sheep_xs1 r = rec[i];
    const uint32_t t = r.tail, h = r.head;
    uint64_t key = dead;
    if (t != h) {
      const uint32_t pt = t < pos_size ? pos[t] : INVALID;
      const uint32_t ph = h < pos_size ? pos[h] : INVALID;
      const bool tin = pt != INVALID && pt < n, hin = ph != INVALID && ph < n;
      if ((tin && h >= pos_size) || (hin && t >= pos_size)) oor = true;
      else if (tin && hin) {
        const uint32_t lo = pt < ph ? pt : ph, hi = pt < ph ? ph : pt;
        const uint32_t d = tD[lo];
        if (d == INVALID) stray = true;   // lo is a root: below nothing
        else key = ((uint64_t)hi << sh) | d;
      }
    }
    keys[i] = key;
  }
  if (__any(oor) && (threadIdx.x & 63) == 0) atomicAdd(&flags[0], 1ull);
  if (__any(stray) && (threadIdx.x & 63) == 0) atomicAdd(&flags[1], 1ull);
}

// Level 0: the node the tour stands on after each arc (a down arc into c: c; an up arc out
// of c: its parent).
__global__ void k_w_level0(const uint32_t *__restrict__ parent, const uint32_t *__restrict__ tD,
                           const uint32_t *__restrict__ tU, uint64_t n, uint32_t *__restrict__ T) {
  const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t c = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; c < n; c += stride) {
    const uint32_t p = parent[c];
    if (p == INVALID) continue;
    T[tD[c]] = (uint32_t)c;
    T[tU[c]] = p;
  }
}

// Level j from level j - 1: the maximum over [i, i + 2^j), for every i with the window inside
// the tour.
__global__ void k_w_level(const uint32_t *__restrict__ prev, uint32_t *__restrict__ cur, uint64_t cnt, uint64_t half) {
  const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < cnt; i += stride) {
    const uint32_t a = prev[i], b = prev[i + half];
    cur[i] = a > b ? a : b;
  }
}

// The lowest common ancestor of the nodes entered at tour positions p <= q.
__device__ __forceinline__ uint32_t tour_lca(const uint32_t *__restrict__ T, uint64_t A, uint32_t p, uint32_t q) {
  const uint32_t len = q - p + 1;
  const int k = 31 - __clz((int)len);
  const uint32_t *row = T + (uint64_t)k * A;
  const uint32_t a = row[p], b = row[q + 1 - (1u << k)];
  return a > b ? a : b;
}

// One pass over the sorted keys.  Entry i of a run of equal hi with tour position p:
//   the next entry has the same hi and the same p (a repeated edge): nothing
//   else +1 at p, and -1 at lca(p, next p) when the run goes on, at hi itself when it ends
// (so every hi with an entry takes its one -1).  Weights land at tour entry positions;
// a root's weight is dropped (its width is 1).
__global__ __launch_bounds__(BLOCK) void k_w_weights(const uint64_t *__restrict__ keys, uint64_t m, int sh, uint64_t n,
                                                     const uint32_t *__restrict__ T, uint64_t A,
                                                     const uint32_t *__restrict__ tD, const uint32_t *__restrict__ ilo,
                                                     const uint32_t *__restrict__ ihi, uint32_t *__restrict__ val,
                                                     unsigned long long *__restrict__ flags) {
  const uint64_t stride = (uint64_t)gridDim.x * BLOCK, dead = (uint64_t)n << sh, mask = ((uint64_t)1 << sh) - 1;
  const uint64_t iters = (m + stride - 1) / stride;
  uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  bool stray = false;
  for (uint64_t it = 0; it < iters; ++it, i += stride) {   // wave-uniform trip count (run_add)
    const uint64_t key = i < m ? keys[i] : dead;
    const uint64_t next = i + 1 < m ? keys[i + 1] : dead;
    const uint64_t hi = key >> sh;
    uint32_t minus = INVALID;
    if (hi < n) {
      const uint32_t p = (uint32_t)(key & mask);
      if (p < ilo[hi] || p >= ihi[hi]) stray = true;
      const bool more = (next >> sh) == hi;
      const uint32_t q = (uint32_t)(next & mask);
      if (p < A && !(more && q == p)) {
        atomicAdd(&val[p], 1u);
        const uint32_t node = more && q < A && q >= p ? tour_lca(T, A, p, q) : (uint32_t)hi;
        if (node < n) minus = tD[node];   // INVALID for a root
      }
    }
    run_add(val, minus, 0xFFFFFFFFu);
  }
  if (__any(stray) && (threadIdx.x & 63) == 0) atomicAdd(&flags[1], 1ull);
}

__global__ void k_w_out(const uint32_t *__restrict__ tD, const uint32_t *__restrict__ tU, uint64_t n,
                        const uint32_t *__restrict__ E, uint32_t *__restrict__ width) {
  const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t v = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; v < n; v += stride) {
    const uint32_t d = tD[v];
    width[v] = d == INVALID ? 1u : 1u + (E[tU[v]] - E[d]);
  }
}

// f[0] = max width, f[1] = sum of (width - pst - 1) in wrapping u64 arithmetic (the
// reference's size_t, jnode.cpp:271), f[2] = the first id with width > 3
__global__ void k_w_facts(const sheep_jnode *__restrict__ tree, const uint32_t *__restrict__ width, uint64_t n,
                          unsigned long long *__restrict__ f) {
  const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
  uint64_t mx = 0, fill = 0, halo = ~0ull;
  for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
    const uint64_t w = width[i];
    mx = w > mx ? w : mx;
    fill += w - (uint64_t)tree[i].pst_weight - 1;
    if (w > 3 && i < halo) halo = i;
  }
  mx = wave_max(mx); fill = wave_sum(fill); halo = wave_min(halo);
  if ((threadIdx.x & 63) == 0) {
    atomicMax(&f[0], (unsigned long long)mx);
    atomicAdd(&f[1], (unsigned long long)fill);
    atomicMin(&f[2], (unsigned long long)halo);
  }
}

int bits_for(uint64_t x) {   // bits that hold every value <= x (at least 1)
  int b = 1;
  while (b < 64 && (x >> b)) ++b;
  return b;
}

}  // namespace

void fill_u32(Ctx &c, uint32_t *p, uint64_t n, uint32_t v);
void tree_facts(Ctx &c, const sheep_jnode *tree, uint64_t n, sheep_facts_t *out);

void tree_widths(Ctx &c, const sheep_xs1 *rec, uint64_t nrec, const uint32_t *pos, uint64_t pos_size,
                 const sheep_jnode *tree, uint64_t n, uint32_t *width) {
  if (n == 0) return;
  if (nrec >= 0xFFFFFFFFull) throw Error(SHEEP_ERR_ARG, "tree_widths: 2^32 records or more");
  TimedRegion all(c, "widths");
  fill_u32(c, width, n, 1u);
  if (nrec == 0) return;
  unsigned long long *flags = c.get_as<unsigned long long>("wd_flags", W_FLAGS);
  HIP_CHECK(hipMemsetAsync(flags, 0, W_FLAGS * sizeof(uint64_t), c.stream));
  sheep_kids k;
  build_kids(c, tree, n, &k);
  try {
    Tour t;
    uint32_t *ilo = c.get_as<uint32_t>("wd_ilo", n), *ihi = c.get_as<uint32_t>("wd_ihi", n);
    {
      TimedRegion tr(c, "widths_tour", 8 * n);
      build_tour(c, &k, t);
      tour_intervals(c, &k, t, ilo, ihi);
    }
    const uint64_t A = t.A;
    const int sh = bits_for(A ? A - 1 : 0), end_bit = sh + bits_for(n);
    uint64_t *keys = c.get_as<uint64_t>("wd_keys", nrec), *kalt = c.get_as<uint64_t>("wd_keys_alt", nrec);
    {
      TimedRegion tr(c, "widths_sort", 12 * nrec + 8 * nrec);
      hipLaunchKernelGGL(k_w_keys, dim3(grid_for(nrec)), dim3(BLOCK), 0, c.stream, rec, nrec, pos, pos_size,
                         (const uint32_t *)t.tD, n, sh, keys, flags);
      LAUNCH_CHECK();
      if (A) {
        bool in_alt = false;
        radix_sort_keys_u64(c, keys, nrec, end_bit, kalt, &in_alt);
        if (in_alt) keys = kalt;
      }
    }
    if (A) {   // (without arcs every node is a root of width 1; an edge there was flagged by k_w_keys)
      const int levels = bits_for(A);   // floor(log2 A) + 1: windows of 1, 2, .. 2^(levels-1) <= A arcs
      uint32_t *T = c.get_as<uint32_t>("wd_lca", A * (uint64_t)levels);
      {
        TimedRegion tr(c, "widths_lca", 8 * A * (uint64_t)levels);
        hipLaunchKernelGGL(k_w_level0, dim3(grid_for(n)), dim3(BLOCK), 0, c.stream, (const uint32_t *)k.parent,
                           (const uint32_t *)t.tD, (const uint32_t *)t.tU, n, T);
        LAUNCH_CHECK();
        for (int j = 1; j < levels; ++j) {
          const uint64_t half = (uint64_t)1 << (j - 1), cnt = A + 1 - 2 * half;
          hipLaunchKernelGGL(k_w_level, dim3(grid_for(cnt)), dim3(BLOCK), 0, c.stream,
                             (const uint32_t *)(T + (uint64_t)(j - 1) * A), T + (uint64_t)j * A, cnt, half);
          LAUNCH_CHECK();
        }
      }
      uint32_t *val = c.get_as<uint32_t>("wd_val", A);
      {
        TimedRegion tr(c, "widths_weights", 8 * nrec);
        HIP_CHECK(hipMemsetAsync(val, 0, A * sizeof(uint32_t), c.stream));
        hipLaunchKernelGGL(k_w_weights, dim3(grid_for(nrec)), dim3(BLOCK), 0, c.stream, (const uint64_t *)keys, nrec, sh,
                           n, (const uint32_t *)T, A, (const uint32_t *)t.tD, (const uint32_t *)ilo,
                           (const uint32_t *)ihi, val, flags);
        LAUNCH_CHECK();
      }
      {
        TimedRegion tr(c, "widths_sums", 8 * A + 12 * n);
        scan_exclusive_u32(c, val, val, A, nullptr);
        hipLaunchKernelGGL(k_w_out, dim3(grid_for(n)), dim3(BLOCK), 0, c.stream, (const uint32_t *)t.tD,
                           (const uint32_t *)t.tU, n, (const uint32_t *)val, width);
        LAUNCH_CHECK();
      }
    }
    uint64_t h[W_FLAGS] = {0, 0};
    c.download(h, (const uint64_t *)flags, W_FLAGS);
    c.sync();
    if (h[0]) throw Error(SHEEP_ERR_RANGE, "tree_widths: vertex id out of range of the sequence index");
    if (h[1])
      throw Error(SHEEP_ERR_ARG, "tree_widths: an edge's earlier end is not below its later end: "
                                 "not the tree of these records and this sequence");
  } catch (...) {
    release_kids(&c, &k);
    throw;
  }
  release_kids(&c, &k);
}

void tree_facts_widths(Ctx &c, const sheep_jnode *tree, uint64_t n, const uint32_t *width, sheep_facts_t *out) {
  tree_facts(c, tree, n, out);
  if (!width || n == 0) return;
  unsigned long long *f = c.get_as<unsigned long long>("wd_facts", 3);
  HIP_CHECK(hipMemsetAsync(f, 0, 2 * sizeof(uint64_t), c.stream));
  HIP_CHECK(hipMemsetAsync(f + 2, 0xFF, sizeof(uint64_t), c.stream));
  hipLaunchKernelGGL(k_w_facts, dim3(grid_for(n)), dim3(BLOCK), 0, c.stream, tree, width, n, f);
  LAUNCH_CHECK();
  uint64_t h[3] = {0, 0, 0};
  c.download(h, (const uint64_t *)f, 3);
  c.sync();
  out->width = h[0];
  out->fill = h[1];
  out->halo_id = h[2] == ~0ull ? INVALID : h[2];
}

}  // namespace sheep
