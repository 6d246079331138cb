// verify.hip — is this forest the elimination tree of these records under this sequence?
// (graph2tree -c; the reference's JTree::isValid, jtree.cpp:238-300, means to ask this but its
// per-edge ancestor walk starts from index.at(X) instead of index.at(nbr) and never runs.)
//
// The certificate.  With the records in sequence positions (lo < hi), a forest over 0..n-1 is
// the elimination tree exactly when
//   1. structure  every parent is INVALID or lies in (v, n);
//   2. descent    for every edge (lo, hi), hi is an ancestor of lo;
//   3. support    every non-root v with parent p has an edge (x, p) with x in v's subtree;
//   4. pst        pst_weight[v] is the count the map defines (etree.hip k_relabel).
// (3) makes every subtree connected, from the leaves up; by (2) every edge that leaves the
// subtree of v ends at a proper ancestor of v, so at p or later: the subtree is a whole component
// of the graph on [0, v] and p is its smallest later neighbour, which is Liu's parent.
// Nothing here calls the tree builder.
//
// Passes (each a TimedRegion under "verify"):
//   verify_structure  over the n nodes.  A failure is final: no kid table and no tour is built
//                     from such a tree, and no later pass reads it.
//   verify_tour       kid table + Euler tour + subtree intervals (tree_tour.hip), kept by the
//                     handle: tD, [ilo, ihi) per node, and kd[j] = tD[kids[j]] per kid slot.
//   verify_records    one pass per record shard: cnt[lo]++ (4), the interval test (2), and for
//                     an edge that passes it the child c of hi whose subtree holds lo gets
//                     sup[c] = 1 (3).  A fresh kid table lists a node's kids in ascending id and
//                     the tour enters them in that order (k_succ walks the CSR segment), so kd is
//                     ascending inside a segment: c is the last kid with kd <= tD[lo], found by
//                     binary search in ceil(log2 kids) steps.
//   verify_finish     over the n nodes: non-roots without a mark, cnt != pst_weight.
// Every index formed from tree or record data is bounded before use: positions by n, kid
// slots by their CSR segment, and the tree's parents by the structure pass.
#include "verify.hpp"

namespace sheep {
namespace {

// Counter words.  A "first" word holds UINT64_MAX - id under atomicMax (0: none), so the
// smallest offender is UINT64_MAX - word whether or not there was one.
enum { V_BAD = 0, V_BAD_FIRST, V_OOR, V_STRAY, V_STRAY_FIRST, V_UNSUP, V_UNSUP_FIRST, V_PST, V_PST_FIRST, V_WORDS };

__global__ __launch_bounds__(BLOCK) void k_v_structure(const sheep_jnode *__restrict__ tree, uint64_t n,
                                                       unsigned long long *__restrict__ ctr) {
  const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
  uint64_t bad = 0, first = 0;
  for (uint64_t v = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; v < n; v += stride) {
    const uint32_t p = tree[v].parent;
    if (p != INVALID && (p <= v || p >= n)) {
      ++bad;
      if (~0ull - v > first) first = ~0ull - v;
    }
  }
  block_atomic_add(&ctr[V_BAD], bad);
  block_atomic_max(&ctr[V_BAD_FIRST], first);
}

__global__ __launch_bounds__(BLOCK) void k_v_records(
    const sheep_xs1 *__restrict__ rec, uint64_t nrec, const uint32_t *__restrict__ pos, uint64_t pos_size, uint64_t n,
    const uint32_t *__restrict__ tD, const uint32_t *__restrict__ ilo, const uint32_t *__restrict__ ihi,
    const uint32_t *__restrict__ koff, const uint32_t *__restrict__ kids, const uint32_t *__restrict__ kd,
    uint32_t *__restrict__ sup, uint32_t *__restrict__ cnt, unsigned long long *__restrict__ ctr) {
  const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
  uint64_t oor = 0, stray = 0, first = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; i < nrec; i += stride) {
    const sheep_xs1 r = rec[i];
    const uint32_t t = r.tail, h = r.head;
    if (t == h) continue;   // a self-loop counts nowhere
    const uint32_t pt = t < pos_size ? pos[t] : INVALID;
    const uint32_t ph = h < pos_size ? pos[h] : INVALID;
    const bool tin = pt != INVALID && pt < n, hin = ph != INVALID && ph < n;
    if ((tin && h >= pos_size) || (hin && t >= pos_size)) { oor = 1; continue; }
    if (tin && hin) {
      if (pt == ph) continue;   // (two vids at one position: not an index of a sequence)
      const uint32_t lo = pt < ph ? pt : ph, hi = pt < ph ? ph : pt;
      atomicAdd(&cnt[lo], 1u);
      const uint32_t d = tD[lo];   // INVALID for a root: in no interval (ihi <= 2n < INVALID)
      uint32_t a = koff[hi], b = koff[hi + 1];
      if (d >= ilo[hi] && d < ihi[hi] && a < b) {
        // kd[a] <= d: hi's interval opens at its first kid's down arc
        while (b - a > 1) {
          const uint32_t m = a + ((b - a) >> 1);
          if (kd[m] <= d) a = m; else b = m;
        }
        const uint32_t c = kids[a];
        if (c < n) sup[c] = 1u;
      } else {
        ++stray;
        if (~0ull - i > first) first = ~0ull - i;
      }
    } else if (tin) {
      atomicAdd(&cnt[pt], 1u);
    } else if (hin) {
      atomicAdd(&cnt[ph], 1u);
    }
  }
  block_atomic_add(&ctr[V_OOR], oor);
  block_atomic_add(&ctr[V_STRAY], stray);
  block_atomic_max(&ctr[V_STRAY_FIRST], first);
}

__global__ __launch_bounds__(BLOCK) void k_v_finish(const sheep_jnode *__restrict__ tree, uint64_t n,
                                                    const uint32_t *__restrict__ sup, const uint32_t *__restrict__ cnt,
                                                    unsigned long long *__restrict__ ctr) {
  const uint64_t stride = (uint64_t)gridDim.x * BLOCK;
  uint64_t unsup = 0, ufirst = 0, pst = 0, pfirst = 0;
  for (uint64_t v = (uint64_t)blockIdx.x * BLOCK + threadIdx.x; v < n; v += stride) {
    const sheep_jnode x = tree[v];
    if (x.parent != INVALID && !sup[v]) {
      ++unsup;
      if (~0ull - v > ufirst) ufirst = ~0ull - v;
    }
    if (cnt[v] != x.pst_weight) {
      ++pst;
      if (~0ull - v > pfirst) pfirst = ~0ull - v;
    }
  }
  block_atomic_add(&ctr[V_UNSUP], unsup);
  block_atomic_max(&ctr[V_UNSUP_FIRST], ufirst);
  block_atomic_add(&ctr[V_PST], pst);
  block_atomic_max(&ctr[V_PST_FIRST], pfirst);
}

}  // namespace

void verify_free(sheep_verify *h) {
  Ctx &c = *h->ctx;
  (void)hipStreamSynchronize(c.stream);   // (queued passes still read the arrays)
  if (h->k.parent) release_kids(&c, &h->k);
  if (h->buf) hipFree(h->buf);
  h->buf = nullptr;
}

// The structure pass and, when it holds, the tour.  h owns everything it keeps: the context's
// tour workspaces belong to the next call on the context (another handle's among them).
void verify_begin(Ctx &c, const sheep_jnode *tree, uint64_t n, sheep_verify *h) {
  h->ctx = &c;
  h->n = n;
  h->tree = tree;
  if (n == 0) return;
  TimedRegion all(c, "verify");
  const uint64_t ctr_bytes = 128;   // V_WORDS u64 and padding: the arrays start on their own line
  static_assert(V_WORDS * sizeof(uint64_t) <= 128, "counter block");
  HIP_CHECK(hipMalloc((void **)&h->buf, ctr_bytes + 6 * (n + 1) * sizeof(uint32_t)));
  h->ctr = (unsigned long long *)h->buf;
  uint32_t *w = (uint32_t *)(h->buf + ctr_bytes);
  h->tD = w; h->ilo = w + (n + 1); h->ihi = w + 2 * (n + 1); h->kd = w + 3 * (n + 1);
  h->sup = w + 4 * (n + 1); h->cnt = w + 5 * (n + 1);
  HIP_CHECK(hipMemsetAsync(h->buf, 0, ctr_bytes, c.stream));
  uint64_t bad[2] = {0, 0};
  {
    TimedRegion tr(c, "verify_structure", 8 * n);
    hipLaunchKernelGGL(k_v_structure, dim3(grid_for(n)), dim3(BLOCK), 0, c.stream, tree, n, h->ctr);
    LAUNCH_CHECK();
    c.download(bad, (const uint64_t *)h->ctr + V_BAD, 2);
    c.sync();
  }
  h->bad_parent = bad[0];
  h->first_bad_parent = ~0ull - bad[1];
  if (h->bad_parent) return;   // final: nothing below may index with these parents
  TimedRegion tr(c, "verify_tour", 8 * n + 24 * n);   // tree read; tD, ilo, ihi, kd, sup, cnt written
  build_kids(c, tree, n, &h->k);
  Tour t;
  build_tour(c, &h->k, t);
  tour_intervals(c, &h->k, t, h->ilo, h->ihi);
  HIP_CHECK(hipMemcpyAsync(h->tD, t.tD, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, c.stream));
  gather_u32(c, t.tD, h->k.kids, h->k.nkids, h->kd);
  HIP_CHECK(hipMemsetAsync(h->sup, 0, 2 * (n + 1) * sizeof(uint32_t), c.stream));   // sup and cnt
  h->toured = true;
}

void verify_add(sheep_verify *h, const sheep_xs1 *rec, uint64_t nrec, const uint32_t *pos, uint64_t pos_size) {
  Ctx &c = *h->ctx;
  if (h->failed) throw Error(SHEEP_ERR_RANGE, "verify: an earlier shard had a vertex id out of range");
  if (!h->toured || nrec == 0) return;   // n == 0, or a structure failure: the verdict is final
  TimedRegion all(c, "verify");
  uint64_t oor = 0;
  {
    // per record: the record (12), both positions (8), cnt (4), tD[lo] (4), hi's interval (8) and
    // CSR segment (8), the kid read (4) and the mark (4); the search's kd reads are not counted
    TimedRegion tr(c, "verify_records", 52 * nrec);
    hipLaunchKernelGGL(k_v_records, dim3(grid_for(nrec)), dim3(BLOCK), 0, c.stream, rec, nrec, pos, pos_size, h->n,
                       (const uint32_t *)h->tD, (const uint32_t *)h->ilo, (const uint32_t *)h->ihi,
                       (const uint32_t *)h->k.koff, (const uint32_t *)h->k.kids, (const uint32_t *)h->kd, h->sup,
                       h->cnt, h->ctr);
    LAUNCH_CHECK();
    c.download(&oor, (const uint64_t *)h->ctr + V_OOR, 1);
    c.sync();
  }
  if (oor) {
    h->failed = true;
    throw Error(SHEEP_ERR_RANGE, "verify: vertex id out of range of the sequence index");
  }
}

void verify_finish(sheep_verify *h, sheep_verify_t *out) {
  Ctx &c = *h->ctx;
  if (h->failed) throw Error(SHEEP_ERR_RANGE, "verify: a shard had a vertex id out of range");
  sheep_verify_t r;
  memset(&r, 0, sizeof r);
  r.bad_parent = h->bad_parent;
  r.first_bad_parent = h->first_bad_parent;
  r.first_not_descendant = r.first_unsupported = r.first_pst_mismatch = ~0ull;
  if (h->toured) {
    TimedRegion all(c, "verify");
    uint64_t w[V_WORDS];
    {
      TimedRegion tr(c, "verify_finish", 8 * h->n + 8 * h->n);
      HIP_CHECK(hipMemsetAsync(h->ctr + V_UNSUP, 0, 4 * sizeof(uint64_t), c.stream));   // finish may run again
      hipLaunchKernelGGL(k_v_finish, dim3(grid_for(h->n)), dim3(BLOCK), 0, c.stream, h->tree, h->n,
                         (const uint32_t *)h->sup, (const uint32_t *)h->cnt, h->ctr);
      LAUNCH_CHECK();
      c.download(w, (const uint64_t *)h->ctr, V_WORDS);
      c.sync();
    }
    r.not_descendant = w[V_STRAY];
    r.first_not_descendant = ~0ull - w[V_STRAY_FIRST];
    r.unsupported = w[V_UNSUP];
    r.first_unsupported = ~0ull - w[V_UNSUP_FIRST];
    r.pst_mismatch = w[V_PST];
    r.first_pst_mismatch = ~0ull - w[V_PST_FIRST];
  }
  r.ok = !r.bad_parent && !r.not_descendant && !r.unsupported && !r.pst_mismatch;
  *out = r;
}

}  // namespace sheep
