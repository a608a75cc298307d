// hostsim (developer tool, never shipped): every kbg::launch_* of
// csrc/kbg_device.hpp — the allocate / backfill / update paths and the
// preempt / reclaim victim scan with its prep — as plain C++ on the simulated
// stream of hostsim_hip.cpp. Each is the contract of csrc/kbg_device.hpp
// restated per node and per row — nothing of the kernels' waves, chunks, LDS
// or rounds — and writes exactly the bytes the kernel writes. A launcher
// copies its argument struct when it is called, as a kernel launch does;
// memory the arguments point to is read when the operation runs.
// tests/test_hostsim_kernels.py holds them to the references the GPU kernels
// are held to (tests/kernel_ref.py, tests/victim_ref.py);
// tests/test_hostsim_victim_why.py does so for the victim-reasons launchers
// (tests/victim_why_ref.py), tests/test_hostsim_task_why.py for the
// pending-task reasons (tests/task_why_ref.py), tests/test_hostsim_headroom.py
// for the pending-task headroom (tests/headroom_ref.py),
// tests/test_hostsim_job_fit.py for the job fit walk (tests/job_fit_ref.py),
// tests/test_hostsim_node_why.py for the node reasons (tests/node_why_ref.py).
//
// The victim launchers count their launches (kbg_hostsim_launch_counts, an
// export of libkbg_hostsim.so alone): tests/test_hostsim_parity.py asserts
// from them that its sessions reached the staged prep, its chunk loop and the
// big-node launch.
#include <algorithm>
#include <atomic>
#include <climits>
#include <cmath>
#include <cstring>
#include <map>
#include <vector>

#include "../csrc/kbg_device.hpp"
#include "hostsim.hpp"

namespace kbg {
namespace {

inline bool le(double r, double a, double mn) { return r < a || std::fabs(a - r) < mn; }  // resource_info.go:142-146

// Resreq.LessEqual(a) for a row's request q (TaskRec: thresholds req - min in integer mode)
inline bool fits(bool int_mode, const double* q, double a0, double a1, double a2) {
  if (int_mode) return a0 > q[0] && a1 > q[1] && a2 > q[2];
  return le(q[0], a0, kMinMilliCPU) && le(q[1], a1, kMinMemory) && le(q[2], a2, kMinMilliGPU);
}

// The node table as one block (FirstFitArgs.nodes) or as NodeSoA pointers.
struct Table {
  const double *ic, *im, *ig, *rc, *rm, *rg;
  const int32_t *nt, *mt;
};
Table table_of(const double* nodes, int32_t stride) {
  const size_t L = (size_t)stride;
  const int32_t* i = reinterpret_cast<const int32_t*>(nodes + 6 * L);
  return Table{nodes, nodes + L, nodes + 2 * L, nodes + 3 * L, nodes + 4 * L, nodes + 5 * L, i, i + L};
}
Table table_of(const NodeSoA& n) {
  return Table{n.idle_cpu, n.idle_mem, n.idle_gpu, n.rel_cpu, n.rel_mem, n.rel_gpu, n.ntasks, n.maxtasks};
}

// One evaluation row against the 64 nodes of global word w: {fits Idle or
// Releasing, fits Idle}, static predicate and pod cap applied. Rows of the
// table are node - tab_lo, nodes outside [tab_lo, tab_lo + tab_n) (tab_n < 0:
// no upper bound) or at / past n_nodes never fit. On a node whose Releasing
// is zero the Releasing fit is the row's kRowRelZeroFits flag.
MaskPair eval_word(const Table& t, const TaskRec& tr, uint64_t static_mask, int32_t w, int32_t n_nodes, int32_t tab_lo,
                   int32_t tab_n, bool cap_check, bool int_mode) {
  MaskPair m{0ull, 0ull};
  for (int b = 0; b < 64; ++b) {
    const int64_t node = (int64_t)w * 64 + b, row = node - tab_lo;
    if (node >= n_nodes || row < 0 || (tab_n >= 0 && row >= tab_n)) continue;
    if (!((static_mask >> b) & 1ull)) continue;
    if (cap_check && !(t.nt[row] < t.mt[row])) continue;  // predicates.go:125-127
    const bool fi = fits(int_mode, tr.req, t.ic[row], t.im[row], t.ig[row]);
    const bool rel_zero = t.rc[row] == 0.0 && t.rm[row] == 0.0 && t.rg[row] == 0.0;
    const bool fr = rel_zero ? (tr.flags & kRowRelZeroFits) != 0 : fits(int_mode, tr.req, t.rc[row], t.rm[row], t.rg[row]);
    if (fi) m.i |= 1ull << b;
    if (fi || fr) m.f |= 1ull << b;
  }
  return m;
}

void firstfit_run(const FirstFitArgs& a, bool int_mode) {
  const Table t = table_of(a.nodes, a.stride);
  // the writer row of each shape, if it has one
  std::vector<char> writer(a.n_shapes, 0);
  if (a.runs) {
    std::fill(writer.begin(), writer.end(), 1);
  } else {
    for (int32_t g = 0; g < a.G; ++g) {
      const uint32_t m = a.row_shape ? a.row_shape[g] : ((uint32_t)g | kRowWriter);
      if (m & kRowWriter) writer[m & ~kRowWriter] = 1;
    }
  }
  for (int32_t s = 0; s < a.n_shapes; ++s) {
    if (!writer[s]) continue;
    const TaskRec tr = a.shapes ? a.shapes[s] : a.inl[s];
    const uint32_t want = a.complete ? 0xffffffffu : ((uint32_t)tr.flags >> kRowWantShift);
    for (int32_t part = 0; part < a.splits; ++part) {
      const int32_t lo = a.w_lo + part * a.split_words, hi = std::min(a.w_hi, lo + a.split_words);
      uint32_t* info = a.info + (size_t)s * a.info_stride + a.part0 + part;
      const int32_t tw = hi - lo;
      if (tw <= 0) {  // no words (a session without nodes)
        *info = 0u;
        if (a.avail) a.avail[s] = 0u;
        continue;
      }
      // the list ends after the word holding its want-th fit; every covered word's masks go out
      MaskPair* out = a.masks + (size_t)s * a.mw - a.mask_w0;
      uint32_t found = 0, covered = 0;
      bool any = false;
      for (int32_t w = lo; w < hi; ++w) {
        // a list that needs nothing (want 0) stays empty; whether a node fits is then
        // reported from the part's first 64 words only
        if (found >= want && !(want == 0 && w - lo < 64)) break;
        const MaskPair m = eval_word(t, tr, a.class_mask[(size_t)tr.cls * a.W + w], w, a.n_nodes, a.tab_lo, a.tab_n,
                                     a.cap_check != 0, int_mode);
        any |= m.f != 0ull;
        if (want == 0) continue;
        out[w] = m;
        covered++;
        found += (uint32_t)__builtin_popcountll(m.f);
      }
      *info = covered | (covered < (uint32_t)tw ? kCountIncompleteBit : 0u) | (any ? kInfoAnyBit : 0u);
      if (a.avail) a.avail[s] = any ? a.avail_bit : 0u;
    }
  }
}

void scan_run(const NodeSoA& n, const ScanGeom& g, const uint64_t* class_mask, const TaskRec* tasks, int32_t n_tasks,
              bool cap_check, bool int_mode, uint64_t* out) {
  const Table t = table_of(n);
  const size_t plane = (size_t)n_tasks * kbg_slot_words(g.Wl);
  for (int32_t rel = 0; rel < g.n_chunks; ++rel) {
    const int32_t chunk = g.chunk_lo + rel;
    if (chunk >= g.W) break;  // words past W are never read or written
    const int32_t slot = rel / g.Wl, w = rel - slot * g.Wl;
    for (int32_t r = 0; r < n_tasks; ++r) {
      const MaskPair m = eval_word(t, tasks[r], class_mask[(size_t)tasks[r].cls * g.W + chunk], chunk, g.n_nodes,
                                   g.tab_lo, -1, cap_check, int_mode);
      uint64_t* o = out + (size_t)slot * 2 * plane + ((size_t)(w >> 2) * n_tasks + r) * 4 + (w & 3);
      o[0] = m.f;
      o[plane] = m.i;
    }
  }
}

// Per row the first M fits of the words [w_lo, w_hi) in node order. The words
// are taken 64 at a time and the walk ends after the group in which the list
// filled, so a list that filled before the last group counts as incomplete
// whether or not a later word holds a fit.
void select_run(const uint64_t* bits, int32_t w_lo, int32_t w_hi, int32_t Wl, int32_t n_rows, const uint32_t* cap_off,
                uint32_t* out_cand, uint32_t* out_count) {
  const size_t plane = (size_t)n_rows * kbg_slot_words(Wl);
  for (int32_t r = 0; r < n_rows; ++r) {
    const int64_t M = (int64_t)cap_off[r + 1] - cap_off[r];
    uint32_t* cand = out_cand + cap_off[r];
    int64_t found = 0;
    int32_t base = w_lo;
    for (; base < w_hi && found < M; base += 64)
      for (int32_t c = base; c < std::min(w_hi, base + 64); ++c) {
        const int32_t slot = c / Wl, w = c - slot * Wl;
        const uint64_t* p = bits + (size_t)slot * 2 * plane + ((size_t)(w >> 2) * n_rows + r) * 4 + (w & 3);
        const uint64_t iw = p[plane];
        for (uint64_t f = p[0]; f; f &= f - 1ull) {
          const int b = __builtin_ctzll(f);
          if (found < M) cand[found] = (uint32_t)(c * 64 + b) | (((iw >> b) & 1ull) ? 0u : kCandPipelineBit);
          ++found;
        }
      }
    const bool complete = base >= w_hi && found <= M;
    out_count[r] = (uint32_t)std::min(found, M) | (complete ? 0u : kCountIncompleteBit);
  }
}

// The node's first decision at or after `point` (its decisions are in log order).
inline int32_t first_undone(const int32_t* hk, int32_t e0, int32_t e1, int32_t point) {
  int32_t lo = e0;
  while (lo < e1 && (hk[lo] & 0x7fffffff) < point) ++lo;
  return lo;
}

void fitdelta_run(const FitArgs& a) {
  const Table t = table_of(a.nodes, a.stride);
  for (int32_t qi = 0; qi < a.nq; ++qi) {
    const FitQuery fq = a.q[qi];
    int32_t cnt[4] = {0, 0, 0, 0};
    const int32_t end = std::min(fq.end, a.tab_lo + a.tab_n);
    for (int32_t n = a.tab_lo; n < end; ++n) {
      if (!((a.class_mask[(size_t)fq.cls * a.W + (n >> 6)] >> (n & 63)) & 1ull)) continue;  // static predicate
      const int32_t r = n - a.tab_lo, e1 = a.hoff[n + 1];
      const int32_t lo = first_undone(a.hk, a.hoff[n], e1, fq.point);
      double c = t.ic[r], m = t.im[r], g = t.ig[r];
      const int32_t x = lo < e1 ? a.na[lo] : -1;  // the first undone Allocate: Idle before it
      if (x >= 0) {
        c = a.hold[3 * (size_t)x];
        m = a.hold[3 * (size_t)x + 1];
        g = a.hold[3 * (size_t)x + 2];
      }
      const bool capped = a.cap_check && t.nt[r] - (e1 - lo) >= t.mt[r];  // pod cap then
      const bool chosen =
          n != fq.win && le(fq.req[0], c, kMinMilliCPU) && le(fq.req[1], m, kMinMemory) && le(fq.req[2], g, kMinMilliGPU);
      if (capped || chosen) continue;
      cnt[0]++;  // Resource.FitDelta (resource_info.go:116-129)
      cnt[1] += (fq.req[0] > 0 ? c - (fq.req[0] + kMinMilliCPU) : c) < 0;
      cnt[2] += (fq.req[1] > 0 ? m - (fq.req[1] + kMinMemory) : m) < 0;
      cnt[3] += (fq.req[2] > 0 ? g - (fq.req[2] + kMinMilliGPU) : g) < 0;
    }
    for (int k = 0; k < 4; ++k) a.out[4 * (size_t)qi + k] = cnt[k];
  }
}

void reasons_run(const ReasonArgs& a) {
  const Table t = table_of(a.nodes, a.stride);
  constexpr int kCode[4] = {0, 1, 3, 4};  // KBG_WHY_* of pod cap, selector, unschedulable, taints
  for (int32_t qi = 0; qi < a.nq; ++qi) {
    const FitQuery fq = a.q[qi];
    const int32_t tab_end = a.tab_lo + a.tab_n;
    const int32_t end = std::min(fq.end, tab_end);
    const int32_t vend = std::min(fq.win >= 0 ? fq.win + 1 : fq.end, tab_end);
    int32_t out[kReasonOut] = {};
    for (int k = 7; k < 13; ++k) out[k] = -1;
    for (int32_t n = a.tab_lo; n < vend; ++n) {
      const uint64_t bit = 1ull << (n & 63);
      const size_t w = (size_t)(n >> 6);
      if (!(a.live[w] & bit)) continue;
      out[0]++;
      if (n >= end || !a.cap_check) continue;  // (the node an Allocate took passed every stage)
      const int32_t r = n - a.tab_lo, e1 = a.hoff[n + 1];
      const bool capped = t.nt[r] - (e1 - first_undone(a.hk, a.hoff[n], e1, fq.point)) >= t.mt[r];
      int s = -1;
      if (capped) s = 0;
      else if (!(a.sel_ok[(size_t)fq.cls * a.W + w] & bit)) s = 1;
      else if (a.unsched[w] & bit) s = 2;
      else if (!(a.taint_ok[(size_t)fq.cls * a.W + w] & bit)) s = 3;
      if (s < 0) continue;
      if (out[1 + kCode[s]]++ == 0) out[7 + kCode[s]] = n;
    }
    std::copy(out, out + kReasonOut, a.out + kReasonOut * (size_t)qi);
  }
}

bool eval_req(const StaticTables& t, const ReqProg& r, int32_t node) {
  switch (r.kind) {
    case REQ_FALSE: return false;
    case REQ_TRUE: return true;
    case REQ_ALL:
    case REQ_ANY:
    case REQ_NONE: {
      bool any = false, all = true;
      for (int32_t w = 0; w < t.label_words; ++w) {
        const uint64_t m = t.mask_pool[r.mask_off + w];
        const uint64_t b = t.label_bits[(size_t)w * t.n_nodes + node] & m;
        any |= b != 0ull;
        all &= b == m;
      }
      return r.kind == REQ_ALL ? all : (r.kind == REQ_ANY ? any : !any);
    }
    case REQ_GT:
    case REQ_LT: {
      const size_t k = (size_t)r.col * t.n_nodes + node;
      if (!t.num_ok[k]) return false;
      return r.kind == REQ_GT ? t.num_vals[k] > r.value : t.num_vals[k] < r.value;
    }
    case REQ_NAME_EQ: return (int64_t)t.name_id[node] == r.value;
    case REQ_NAME_NE: return (int64_t)t.name_id[node] != r.value;
  }
  return false;
}

// nodeSelector and required node affinity (vendor predicates.go:807-850)
bool selector_ok(const StaticTables& t, const ClassProg& c, int32_t node) {
  if (c.sel_req >= 0 && !eval_req(t, t.reqs[c.sel_req], node)) return false;
  if (!c.has_affinity) return true;
  for (int32_t i = 0; i < c.term_len; ++i) {
    const TermProg tp = t.terms[c.term_off + i];
    bool all = true;
    for (int32_t j = 0; j < tp.req_len && all; ++j) all = eval_req(t, t.reqs[tp.req_off + j], node);
    if (all) return true;
  }
  return false;
}
// every taint tolerated (vendor predicates.go:1489-1517)
bool taints_ok(const StaticTables& t, const ClassProg& c, int32_t node) {
  for (int32_t w = 0; w < t.taint_words; ++w)
    if (t.taint_bits[(size_t)w * t.n_nodes + node] & ~t.tol_pool[c.tol_off + w]) return false;
  return true;
}

void class_mask_run(const StaticTables& t, int32_t n_classes, int32_t W, uint64_t* class_mask) {
  for (int32_t cls = 0; cls < n_classes; ++cls) {
    const ClassProg c = t.classes[cls];
    for (int32_t w = 0; w < W; ++w) {
      uint64_t m = 0ull;
      for (int b = 0; b < 64; ++b) {
        const int32_t node = w * 64 + b;
        if (node >= t.n_nodes) break;
        const uint8_t fl = t.node_flags[node];
        bool ok;
        if (c.always || (fl & NF_NIL)) ok = true;  // a nil Node: the host reports it when reached
        else if (fl & (NF_UNSCHED | NF_DEAD)) ok = false;
        else ok = selector_ok(t, c, node) && taints_ok(t, c, node);
        if (ok) m |= 1ull << b;
      }
      class_mask[(size_t)cls * W + w] = m;
    }
  }
}

void stage_planes_run(const StaticTables& t, int32_t n_classes, int32_t W, const StagePlanes& p) {
  for (int32_t cls = 0; cls < n_classes; ++cls) {
    const ClassProg c = t.classes[cls];
    for (int32_t w = 0; w < W; ++w) {
      uint64_t ms = 0, mt = 0, mu = 0, ml = 0;
      for (int b = 0; b < 64; ++b) {
        const int32_t node = w * 64 + b;
        if (node >= t.n_nodes) break;
        const uint8_t fl = t.node_flags[node];
        const bool nil = (fl & NF_NIL) != 0;  // passes every stage here
        if (nil || !(fl & NF_DEAD)) ml |= 1ull << b;
        if (!nil && (fl & NF_UNSCHED)) mu |= 1ull << b;
        const bool plain = c.always || nil;
        if (plain || selector_ok(t, c, node)) ms |= 1ull << b;
        if (plain || taints_ok(t, c, node)) mt |= 1ull << b;
      }
      p.sel_ok[(size_t)cls * W + w] = ms;
      p.taint_ok[(size_t)cls * W + w] = mt;
      if (cls == 0) {
        p.unsched[w] = mu;
        p.live[w] = ml;
      }
    }
  }
}

// ---- preempt / reclaim victim scan (preempt.go:182-240, reclaim.go:106-135)
inline bool le3(const double* r, const double* a) {  // Resource.LessEqual
  return le(r[0], a[0], kMinMilliCPU) && le(r[1], a[1], kMinMemory) && le(r[2], a[2], kMinMilliGPU);
}
// Resource.Less
inline bool less3(const double* a, const double* b) { return a[0] < b[0] && a[1] < b[1] && a[2] < b[2]; }
// Resource.Sub (resource_info.go:100-110): false where the reference panics
inline bool sub3(double* a, const double* r) {
  const bool ok = le3(r, a);
  for (int d = 0; d < 3; ++d) a[d] -= r[d];
  return ok;
}
// drf.go:156-166 with helpers.Share
inline double share3(const double* a, const double* tot) {
  double res = 0;
  for (int d = 0; d < 3; ++d) {
    const double s = tot[d] == 0 ? (a[d] == 0 ? 0.0 : 1.0) : a[d] / tot[d];
    if (s > res) res = s;
  }
  return res;
}

struct Alloc3 {
  double v[3];
};
// A victim fn's running allocation of job / queue `id`, starting from the table's row.
inline double* running(std::map<int32_t, Alloc3>& m, int32_t id, const double* table) {
  auto it = m.find(id);
  if (it == m.end()) {
    const double* row = table + 3 * (size_t)id;
    it = m.emplace(id, Alloc3{{row[0], row[1], row[2]}}).first;
  }
  return it->second.v;
}

enum Verdict : int { kMoveOn = 0, kStop = 1, kPanic = 2 };

// What the reference does when the preemptor reaches the node of table row
// `row`: PredicateFn (static class bit, the nil-node panic, the pod cap), the
// action's preemptee filter over the node's Running candidates in
// NodeInfo.Tasks order, the victim fns of the first tier that yields a victim
// (gang.go:104-124, drf.go:80-105, proportion.go:161-186, intersected:
// session_plugins.go:59-140) and validateVictims (preempt.go:242-253).
Verdict victim_verdict(const VictimScan& p, const VictimTables& t, int32_t row) {
  const int32_t n = p.node_lo + row;
  if (!((t.class_mask[(size_t)p.cls * p.W + (n >> 6)] >> (n & 63)) & 1ull)) return kMoveOn;
  if (t.panic_node[n]) return kPanic;                                       // predicates.go:122-123
  if (p.cap_check && t.ntasks[row] >= t.maxtasks[row]) return kMoveOn;      // :125-127
  const int32_t* jq = reinterpret_cast<const int32_t*>(t.c_jq);
  std::vector<size_t> pre;  // candidate positions
  for (size_t pos = (size_t)t.nt_off[n]; pos < (size_t)t.nt_off[n + 1]; ++pos) {
    if (!t.c_run[pos]) continue;
    const int32_t job = jq[2 * pos], queue = jq[2 * pos + 1];
    bool f;
    if (p.mode == VM_PREEMPT_JOBS) f = queue == p.queue && job != p.job;  // preempt.go:100-112
    else if (p.mode == VM_PREEMPT_TASKS) f = job == p.job;                // :146-154
    else f = queue != p.queue;                                            // reclaim.go:113-126
    if (f) pre.push_back(pos);
  }
  if (pre.empty()) return kMoveOn;
  std::vector<size_t> victims;
  for (int32_t ti = 0; ti < p.n_tiers && victims.empty(); ++ti) {
    const int32_t fns = p.tier_fns[ti];
    std::vector<char> keep(pre.size(), 1);
    if (fns & VP_GANG)
      for (size_t i = 0; i < pre.size(); ++i) {
        const int32_t job = jq[2 * pre[i]];
        if (!(t.j_min[job] <= t.j_ready[job] - 1)) keep[i] = 0;
      }
    if (fns & VP_DRF) {  // every preemptee subtracts from its job, in order, whatever the other fns keep
      std::map<int32_t, Alloc3> alloc;
      for (size_t i = 0; i < pre.size(); ++i) {
        double* a = running(alloc, jq[2 * pre[i]], t.j_alloc);
        if (!sub3(a, t.c_req + 3 * pre[i])) return kPanic;
        const double rs = share3(a, t.drf_total);
        if (!(p.ls < rs || std::fabs(p.ls - rs) <= 0.000001)) keep[i] = 0;
      }
    }
    if (fns & VP_PROP) {
      std::map<int32_t, Alloc3> alloc;
      for (size_t i = 0; i < pre.size(); ++i) {
        const int32_t queue = jq[2 * pre[i] + 1];
        const double* r = t.c_req + 3 * pre[i];
        double* a = running(alloc, queue, t.q_alloc);
        if (less3(a, r)) {  // skipped: the allocation stays
          keep[i] = 0;
          continue;
        }
        if (!sub3(a, r)) return kPanic;
        if (!le3(t.q_deserved + 3 * (size_t)queue, a)) keep[i] = 0;
      }
    }
    for (size_t i = 0; i < pre.size(); ++i)
      if (keep[i]) victims.push_back(pre[i]);
  }
  if (victims.empty()) return kMoveOn;
  double all[3] = {0.0, 0.0, 0.0};  // validateVictims, in victims order
  for (size_t pos : victims)
    for (int d = 0; d < 3; ++d) all[d] += t.c_req[3 * pos + d];
  return less3(all, p.req) ? kMoveOn : kStop;
}

inline int32_t candidates_of(const VictimScan& p, const VictimTables& t, int32_t row) {
  return t.nt_off[p.node_lo + row + 1] - t.nt_off[p.node_lo + row];
}

// The stop and panic bits of the range's nodes, a byte (8 nodes) at a time:
// every byte holding a node of the range is written whole, bits past the
// range 0, and so is the bit of a node holding more than 128 candidates
// (launch_victim_big's). No other byte is touched.
void victim_scan_run(const VictimScan& p, const VictimTables& t, uint32_t* stop_bits, uint32_t* panic_bits) {
  uint8_t* stop = reinterpret_cast<uint8_t*>(stop_bits) + (p.node_lo >> 3);
  uint8_t* panic = reinterpret_cast<uint8_t*>(panic_bits) + (p.node_lo >> 3);
  for (int32_t r0 = 0; r0 < p.node_n; r0 += 8) {
    uint8_t s = 0, q = 0;
    for (int32_t row = r0; row < std::min(p.node_n, r0 + 8); ++row) {
      if (candidates_of(p, t, row) > 128) continue;
      const Verdict v = victim_verdict(p, t, row);
      if (v != kMoveOn) s |= (uint8_t)(1u << (row - r0));
      if (v == kPanic) q |= (uint8_t)(1u << (row - r0));
    }
    stop[r0 >> 3] = s;
    panic[r0 >> 3] = q;
  }
}

void victim_big_run(const VictimScan& p, const VictimTables& t, const int32_t* rows, int32_t n_rows,
                    uint32_t* stop_bits, uint32_t* panic_bits, uint8_t* row_out) {
  for (int32_t i = 0; i < n_rows; ++i) {
    const Verdict v = victim_verdict(p, t, rows[i]);
    if (row_out) {
      row_out[i] = v == kMoveOn ? 0u : v == kStop ? 1u : 3u;  // bit 0 stop, bit 1 panic
      continue;
    }
    if (v == kMoveOn) continue;
    const int32_t n = p.node_lo + rows[i];
    stop_bits[n >> 5] |= 1u << (n & 31);
    if (v == kPanic) panic_bits[n >> 5] |= 1u << (n & 31);
  }
}

// ---- victim reasons (kbg_device.hpp VictimWhy): the cause of table row `row`
// for query p, per node, and the fns of a walked tier whose own result over
// the whole preemptee list is empty (VictimPlugin bits in *fn_empty, set for
// kWhyNoVictims only). The node is live.
int32_t victim_why_cause(const VictimWhyArgs& a, const VictimScan& p, const VictimTables& t, int32_t row,
                         int32_t* fn_empty) {
  *fn_empty = 0;
  const int32_t n = a.node_lo + row;
  const uint64_t bit = 1ull << (n & 63);
  if (t.panic_node[n]) return kWhyPanic;  // predicates.go:122-123
  if (p.cap_check) {                      // :125-183, the first failing stage
    if (t.ntasks[row] >= t.maxtasks[row]) return 0;
    if (!(a.sel_ok[(size_t)p.cls * a.W + (n >> 6)] & bit)) return 1;
    if (a.unsched[n >> 6] & bit) return 3;
    if (!(a.taint_ok[(size_t)p.cls * a.W + (n >> 6)] & bit)) return 4;
  }
  const int32_t* jq = reinterpret_cast<const int32_t*>(t.c_jq);
  std::vector<size_t> pre;
  for (size_t pos = (size_t)t.nt_off[n]; pos < (size_t)t.nt_off[n + 1]; ++pos) {
    if (!t.c_run[pos]) continue;
    const int32_t job = jq[2 * pos], queue = jq[2 * pos + 1];
    bool f;
    if (p.mode == VM_PREEMPT_JOBS) f = queue == p.queue && job != p.job;
    else if (p.mode == VM_PREEMPT_TASKS) f = job == p.job;
    else f = queue != p.queue;
    if (f) pre.push_back(pos);
  }
  if (pre.empty()) return kWhyNoPreemptees;
  int32_t empty = 0;
  for (int32_t ti = 0; ti < p.n_tiers; ++ti) {
    const int32_t fns = p.tier_fns[ti];
    std::vector<char> kg(pre.size(), 1), kd(pre.size(), 1), kp(pre.size(), 1);
    if (fns & VP_GANG)
      for (size_t i = 0; i < pre.size(); ++i) {
        const int32_t job = jq[2 * pre[i]];
        kg[i] = t.j_min[job] <= t.j_ready[job] - 1;
      }
    if (fns & VP_DRF) {
      std::map<int32_t, Alloc3> alloc;
      for (size_t i = 0; i < pre.size(); ++i) {
        double* al = running(alloc, jq[2 * pre[i]], t.j_alloc);
        if (!sub3(al, t.c_req + 3 * pre[i])) return kWhyPanic;
        const double rs = share3(al, t.drf_total);
        kd[i] = p.ls < rs || std::fabs(p.ls - rs) <= 0.000001;
      }
    }
    if (fns & VP_PROP) {
      std::map<int32_t, Alloc3> alloc;
      for (size_t i = 0; i < pre.size(); ++i) {
        const int32_t queue = jq[2 * pre[i] + 1];
        const double* r = t.c_req + 3 * pre[i];
        double* al = running(alloc, queue, t.q_alloc);
        if (less3(al, r)) {  // skipped: the allocation stays
          kp[i] = 0;
          continue;
        }
        if (!sub3(al, r)) return kWhyPanic;
        kp[i] = le3(t.q_deserved + 3 * (size_t)queue, al);
      }
    }
    auto none = [](const std::vector<char>& k) { return std::find(k.begin(), k.end(), 1) == k.end(); };
    if ((fns & VP_GANG) && none(kg)) empty |= VP_GANG;
    if ((fns & VP_DRF) && none(kd)) empty |= VP_DRF;
    if ((fns & VP_PROP) && none(kp)) empty |= VP_PROP;
    double all[3] = {0.0, 0.0, 0.0};  // validateVictims, in victims order
    bool some = false;
    for (size_t i = 0; i < pre.size(); ++i)
      if (kg[i] && kd[i] && kp[i]) {
        some = true;
        for (int d = 0; d < 3; ++d) all[d] += t.c_req[3 * pre[i] + d];
      }
    if (some) return less3(all, p.req) ? kWhyNotEnough : kWhyVictims;
  }
  *fn_empty = empty;
  return kWhyNoVictims;
}

void victim_why_add(const VictimWhyArgs& a, const VictimTables& t, int32_t q, int32_t row) {
  const int32_t n = a.node_lo + row;
  if (!((a.live[n >> 6] >> (n & 63)) & 1ull)) return;
  int32_t fn_empty = 0;
  const int32_t c = victim_why_cause(a, a.q[q], t, row, &fn_empty);
  int32_t* o = a.out + (size_t)q * kVictimWhyOut;
  o[c]++;
  if (o[kWhyCauses + c] < 0 || n < o[kWhyCauses + c]) o[kWhyCauses + c] = n;
  for (int f = 0; f < 3; ++f)
    if ((fn_empty >> f) & 1) o[2 * kWhyCauses + f]++;
}

// Every row gets its empty value, then the live nodes of up to 128 candidates.
void victim_why_run(const VictimWhyArgs& a, const VictimTables& t) {
  for (int32_t q = 0; q < a.nq; ++q) {
    int32_t* o = a.out + (size_t)q * kVictimWhyOut;
    std::fill(o, o + kVictimWhyOut, 0);
    std::fill(o + kWhyCauses, o + 2 * kWhyCauses, -1);
    for (int32_t row = 0; row < a.node_n; ++row)
      if (t.nt_off[a.node_lo + row + 1] - t.nt_off[a.node_lo + row] <= 128) victim_why_add(a, t, q, row);
  }
}

// The listed rows of 129..kMaxNodeCandidates candidates, added to the rows.
void victim_why_big_run(const VictimWhyArgs& a, const VictimTables& t, const int32_t* rows, int32_t n_rows) {
  for (int32_t q = 0; q < a.nq; ++q)
    for (int32_t i = 0; i < n_rows; ++i) {
      const int32_t L = t.nt_off[a.node_lo + rows[i] + 1] - t.nt_off[a.node_lo + rows[i]];
      if (L > 128 && L <= kMaxNodeCandidates) victim_why_add(a, t, q, rows[i]);
    }
}

// ---- pending-task reasons (kbg_device.hpp TaskWhy): the cause of table row
// `row` for shape sh, and the dimensions in which Idle.FitDelta(req) is
// negative (bits 0..2 of *idle_short, set for causes 7 and 8 only). The node is
// live and inside the table.
int32_t task_why_cause(const TaskWhyArgs& a, const Table& t, const TaskShape& sh, int32_t row, int32_t* idle_short) {
  *idle_short = 0;
  const int32_t n = a.tab_lo + row;
  const uint64_t bit = 1ull << (n & 63);
  if (a.cap_check) {  // predicates.go:125-183, the first failing stage
    if (t.nt[row] >= t.mt[row]) return 0;
    if (!(a.sel_ok[(size_t)sh.cls * a.W + (n >> 6)] & bit)) return 1;
    if (a.unsched[n >> 6] & bit) return 3;
    if (!(a.taint_ok[(size_t)sh.cls * a.W + (n >> 6)] & bit)) return 4;
  }
  if (sh.flags & kTaskShapeBestEffort) return kTwhyFitsIdle;  // backfill.go:47-60: no resource test
  if (fits(false, sh.req, t.ic[row], t.im[row], t.ig[row])) return kTwhyFitsIdle;
  const double idle[3] = {t.ic[row], t.im[row], t.ig[row]};
  const double mn[3] = {kMinMilliCPU, kMinMemory, kMinMilliGPU};
  for (int d = 0; d < 3; ++d)  // Resource.FitDelta (resource_info.go:116-129)
    if ((sh.req[d] > 0 ? idle[d] - (sh.req[d] + mn[d]) : idle[d]) < 0) *idle_short |= 1 << d;
  return fits(false, sh.req, t.rc[row], t.rm[row], t.rg[row]) ? kTwhyFitsReleasing : kTwhyShort;
}

void task_why_init_run(int32_t* out, int32_t n_shapes) {
  for (int32_t s = 0; s < n_shapes; ++s) {
    int32_t* o = out + (size_t)s * kTaskWhyOut;
    std::fill(o, o + kTaskWhyOut, 0);
    std::fill(o + kTwhyCauses, o + 2 * kTwhyCauses, -1);
  }
}

void task_why_run(const TaskWhyArgs& a) {
  const Table t = table_of(a.nodes, a.stride);
  for (int32_t s = 0; s < a.n_shapes; ++s) {
    int32_t* o = a.out + (size_t)s * kTaskWhyOut;
    for (int32_t row = 0; row < a.tab_n; ++row) {
      const int32_t n = a.tab_lo + row;
      if (!((a.live[n >> 6] >> (n & 63)) & 1ull)) continue;
      int32_t idle_short = 0;
      const int32_t c = task_why_cause(a, t, a.shapes[s], row, &idle_short);
      o[c]++;
      if (o[kTwhyCauses + c] < 0 || n < o[kTwhyCauses + c]) o[kTwhyCauses + c] = n;
      for (int d = 0; d < 3; ++d)
        if ((idle_short >> d) & 1) o[2 * kTwhyCauses + d]++;
    }
  }
}

// ---- node reasons (kbg_device.hpp NodeWhy): the slots [0, 64 * n_words) of
// every plane get their empty value; then each listed word's live rows inside
// the table take every shape record under task_why_cause's cause.
void node_why_init_run(int32_t* out, int32_t ostride, int32_t n_words) {
  for (int f = 0; f < kNodeWhyFields; ++f)
    std::fill_n(out + (size_t)f * ostride, (size_t)n_words * 64, f >= kNwhyFirst && f < kNwhyShort ? -1 : 0);
}

void node_why_run(const NodeWhyArgs& a) {
  const Table t = table_of(a.nodes, a.stride);
  TaskWhyArgs ta{};
  ta.W = a.W;
  ta.tab_lo = a.tab_lo;
  ta.sel_ok = a.sel_ok;
  ta.taint_ok = a.taint_ok;
  ta.unsched = a.unsched;
  ta.cap_check = a.cap_check;
  const size_t P = (size_t)a.ostride;
  for (int32_t i = 0; i < a.n_words; ++i)
    for (int32_t l = 0; l < 64; ++l) {
      const int32_t row = a.words[i] * 64 + l, n = a.tab_lo + row;
      if (row >= a.tab_n || !((a.live[n >> 6] >> (n & 63)) & 1ull)) continue;
      int32_t* o = a.out + (size_t)i * 64 + l;
      for (int32_t s = 0; s < a.n_shapes; ++s) {
        const NodeWhyShape& r = a.shapes[s];
        int32_t idle_short = 0;
        const int32_t c = task_why_cause(ta, t, r.sh, row, &idle_short);
        int k = 0;
        while (kNodeWhyCause[k] != c) ++k;
        o[(kNwhyCount + k) * P] += r.weight;
        int32_t& first = o[(kNwhyFirst + k) * P];
        if (first < 0 || r.first_task < first) first = r.first_task;
        for (int d = 0; d < 3; ++d)
          if ((idle_short >> d) & 1) o[(kNwhyShort + d) * P] += r.weight;
        if (c == kTwhyFitsIdle) {
          o[kNwhyOpenIdle * P] += r.weight_open;
          if (r.sh.flags & kTaskShapeBestEffort) o[kNwhyIdleBestEffort * P] += r.weight;
        } else if (c == kTwhyFitsReleasing) {
          o[kNwhyOpenRel * P] += r.weight_open;
        }
      }
    }
}

// ---- pending-task headroom (kbg_device.hpp TaskRoom): the copies of shape sh
// table row `row` takes one after the other, {from Idle, from Releasing}, with
// *pass whether the node is past the stages and *cut whether `limit` ended the
// count below the node's pod room. The node is live and inside the table.
std::pair<int32_t, int32_t> task_room_node(const TaskRoomArgs& a, const Table& t, const TaskShape& sh, int32_t row,
                                           bool* pass, bool* cut) {
  *pass = *cut = false;
  const int32_t n = a.tab_lo + row;
  const uint64_t bit = 1ull << (n & 63);
  int64_t room = INT32_MAX;
  if (a.cap_check) {  // predicates.go:125-183
    if (t.nt[row] >= t.mt[row]) return {0, 0};
    if (!(a.sel_ok[(size_t)sh.cls * a.W + (n >> 6)] & bit)) return {0, 0};
    if (a.unsched[n >> 6] & bit) return {0, 0};
    if (!(a.taint_ok[(size_t)sh.cls * a.W + (n >> 6)] & bit)) return {0, 0};
    room = (int64_t)t.mt[row] - t.nt[row];
  }
  *pass = true;
  const int32_t bound = (int32_t)std::min<int64_t>(a.limit, room);
  int32_t i = 0, k_idle;
  if (sh.flags & kTaskShapeBestEffort) {  // backfill.go:47-60: no resource test
    i = k_idle = bound;
  } else {
    double x[3] = {t.ic[row], t.im[row], t.ig[row]};
    for (; i < bound && fits(false, sh.req, x[0], x[1], x[2]); ++i)  // Idle.Sub (node_info.go:108-118)
      for (int d = 0; d < 3; ++d) x[d] -= sh.req[d];
    k_idle = i;
    double y[3] = {t.rc[row], t.rm[row], t.rg[row]};
    for (; i < bound && fits(false, sh.req, y[0], y[1], y[2]); ++i)  // Releasing.Sub (node_info.go:119-126)
      for (int d = 0; d < 3; ++d) y[d] -= sh.req[d];
  }
  *cut = i == a.limit && a.limit < room;
  return {k_idle, i - k_idle};
}

void task_headroom_init_run(int32_t* out, int32_t n_shapes) {
  for (int32_t s = 0; s < n_shapes; ++s) {
    int32_t* o = out + (size_t)s * kRoomOut;
    std::fill(o, o + kRoomOut, 0);
    o[kRoomFirstNode] = -1;
  }
}

void task_headroom_run(const TaskRoomArgs& a) {
  const Table t = table_of(a.nodes, a.stride);
  for (int32_t s = 0; s < a.n_shapes; ++s) {
    int32_t* o = a.out + (size_t)s * kRoomOut;
    for (int32_t row = 0; row < a.tab_n; ++row) {
      const int32_t n = a.tab_lo + row;
      if (!((a.live[n >> 6] >> (n & 63)) & 1ull)) continue;
      bool pass, cut;
      const auto [k_idle, k_rel] = task_room_node(a, t, a.shapes[s], row, &pass, &cut);
      if (!pass) continue;
      o[kRoomNodesPass]++;
      o[kRoomCopiesIdle] += k_idle;
      o[kRoomCopiesRel] += k_rel;
      if (k_idle > 0) o[kRoomNodesIdle]++;
      if (k_idle == 0 && k_rel > 0) o[kRoomNodesRelOnly]++;
      if (k_idle + k_rel > 0 && (o[kRoomFirstNode] < 0 || n < o[kRoomFirstNode])) o[kRoomFirstNode] = n;
      o[kRoomMaxNodeCopies] = std::max(o[kRoomMaxNodeCopies], k_idle + k_rel);
      if (cut) o[kRoomLimitHit]++;
    }
  }
}

// ---- job fit walk (kbg_device.hpp JobFitArgs): every job's steps in order
// against a view of its own, a map of the rows its walk has touched. The
// cursor is the device's: a step starts at the row its prev landed on.
void job_fit_run(const JobFitArgs& a) {
  const Table t = table_of(a.nodes, a.stride);
  struct View {
    double idle[3], rel[3];
    int32_t nt;
  };
  for (int32_t j = 0; j < a.n_jobs; ++j) {
    const int32_t s0 = a.job_off[j], ns = a.job_off[j + 1] - s0;
    std::map<int32_t, View> view;
    std::vector<int32_t> land(ns, -1);
    for (int32_t i = 0; i < ns; ++i) {
      const JobFitStep& st = a.steps[s0 + i];
      const TaskShape& sh = a.shapes[st.shape];
      int32_t at = -1, kind = 0;
      const int32_t from = st.prev >= 0 ? land[st.prev] : 0;
      for (int32_t row = from; from >= 0 && row < a.tab_n; ++row) {
        const int32_t n = a.tab_lo + row;
        const uint64_t bit = 1ull << (n & 63);
        if (!(a.live[n >> 6] & bit)) continue;
        View v{{t.ic[row], t.im[row], t.ig[row]}, {t.rc[row], t.rm[row], t.rg[row]}, t.nt[row]};
        const auto it = view.find(row);
        if (it != view.end()) v = it->second;
        if (a.cap_check) {  // predicates.go:125-183
          if (v.nt >= t.mt[row]) continue;
          if (!(a.sel_ok[(size_t)sh.cls * a.W + (n >> 6)] & bit)) continue;
          if (a.unsched[n >> 6] & bit) continue;
          if (!(a.taint_ok[(size_t)sh.cls * a.W + (n >> 6)] & bit)) continue;
        }
        double* x = nullptr;
        if (fits(false, sh.req, v.idle[0], v.idle[1], v.idle[2])) x = v.idle, kind = 0;  // allocate.go:136-146
        else if (fits(false, sh.req, v.rel[0], v.rel[1], v.rel[2])) x = v.rel, kind = 1;  // allocate.go:148-162
        if (!x) continue;
        for (int d = 0; d < 3; ++d) x[d] -= sh.req[d];
        v.nt++;
        view[row] = v;
        at = row;
        break;
      }
      land[i] = at;
      a.out[2 * (size_t)(s0 + i)] = at < 0 ? -1 : a.tab_lo + at;
      a.out[2 * (size_t)(s0 + i) + 1] = at < 0 ? 0 : kind;
    }
  }
}

// ---- node drain walk (kbg_device.hpp DrainArgs): job_fit_run's walk with the
// launch's excluded plane, each walk's own excluded row and BestEffort steps.
void drain_run(const DrainArgs& a) {
  const Table t = table_of(a.nodes, a.stride);
  struct View {
    double idle[3], rel[3];
    int32_t nt;
  };
  for (int32_t j = 0; j < a.n_walks; ++j) {
    const int32_t s0 = a.walk_off[j], ns = a.walk_off[j + 1] - s0, xrow = a.walk_row[j];
    std::map<int32_t, View> view;
    std::vector<int32_t> land(ns, -1);
    for (int32_t i = 0; i < ns; ++i) {
      const JobFitStep& st = a.steps[s0 + i];
      const TaskShape& sh = a.shapes[st.shape];
      const bool beff = (sh.flags & kTaskShapeBestEffort) != 0;
      int32_t at = -1, kind = 0;
      const int32_t from = st.prev >= 0 ? land[st.prev] : 0;
      for (int32_t row = from; from >= 0 && row < a.tab_n; ++row) {
        const int32_t n = a.tab_lo + row;
        const uint64_t bit = 1ull << (n & 63);
        if (!(a.live[n >> 6] & bit) || (a.excl[n >> 6] & bit) || row == xrow) continue;
        View v{{t.ic[row], t.im[row], t.ig[row]}, {t.rc[row], t.rm[row], t.rg[row]}, t.nt[row]};
        const auto it = view.find(row);
        if (it != view.end()) v = it->second;
        if (a.cap_check) {  // predicates.go:125-183
          if (v.nt >= t.mt[row]) continue;
          if (!(a.sel_ok[(size_t)sh.cls * a.W + (n >> 6)] & bit)) continue;
          if (a.unsched[n >> 6] & bit) continue;
          if (!(a.taint_ok[(size_t)sh.cls * a.W + (n >> 6)] & bit)) continue;
        }
        double* x = nullptr;
        if (beff) x = v.idle, kind = 0;  // backfill.go:47-64: no resource test
        else if (fits(false, sh.req, v.idle[0], v.idle[1], v.idle[2])) x = v.idle, kind = 0;  // allocate.go:136-146
        else if (fits(false, sh.req, v.rel[0], v.rel[1], v.rel[2])) x = v.rel, kind = 1;  // allocate.go:148-162
        if (!x) continue;
        for (int d = 0; d < 3; ++d) x[d] -= sh.req[d];
        v.nt++;
        view[row] = v;
        at = row;
        break;
      }
      land[i] = at;
      a.out[2 * (size_t)(s0 + i)] = at < 0 ? -1 : a.tab_lo + at;
      a.out[2 * (size_t)(s0 + i) + 1] = at < 0 ? 0 : kind;
    }
  }
}

void node_delta_run(const NodeSoA& n, const NodeDelta& d) {
  n.idle_cpu[d.node] = d.idle[0];
  n.idle_mem[d.node] = d.idle[1];
  n.idle_gpu[d.node] = d.idle[2];
  n.rel_cpu[d.node] = d.rel[0];
  n.rel_mem[d.node] = d.rel[1];
  n.rel_gpu[d.node] = d.rel[2];
  n.ntasks[d.node] = d.ntasks;
  n.maxtasks[d.node] = d.maxtasks;
}

void victim_prep_run(const NodeSoA& n, const VictimTables& t, const NodeDelta* nd, int32_t nn, const StateDelta* sd,
                     int32_t ns) {
  for (int32_t i = 0; i < nn; ++i) node_delta_run(n, nd[i]);
  for (int32_t i = 0; i < ns; ++i) {
    const StateDelta& x = sd[i];
    switch (x.kind) {
      case 0: t.c_run[x.index] = (uint8_t)(x.v[0] != 0.0); break;
      case 1: t.j_ready[x.index] = (int32_t)x.v[0]; break;
      case 2: std::copy(x.v, x.v + 3, t.j_alloc + 3 * (size_t)x.index); break;
      case 3: std::copy(x.v, x.v + 3, t.q_alloc + 3 * (size_t)x.index); break;
    }
  }
}

// Launch counters of the victim launchers (kbg_hostsim_launch_counts).
enum Count : int {
  kCountScan,
  kCountBig,
  kCountBigRowOut,
  kCountPrep,
  kCountPrepNextChunk,
  kCountPrepInline,
  kCountPrepInlineNodes,
  kCountPrepInlineState,
  kCountTaskWhy,
  kCountTaskHeadroom,
  kCountStageMask,
  kCountNodeWhy,  // (ahead of the last two: tests/test_hostsim_job_fit.py names the list's end)
  kCountDrain,    // (after node_why, for the same reason)
  kCountVictimWhy,
  kCountJobFit,
  kCounts
};
constexpr const char* kCountNames =
    "victim_scan,victim_big,victim_big_row_out,victim_prep,victim_prep_next_chunk,victim_prep_inline,"
    "victim_prep_inline_nodes,victim_prep_inline_state,task_why,task_headroom,stage_mask,node_why,drain,victim_why,job_fit";
std::atomic<int64_t> g_count[kCounts];
// Every launch of this file in order, and the staged prep's last one: a
// staged prep that directly follows a staged prep and carries node rows, or
// follows one that filled its state staging, is the next chunk of the same
// victim_push (the first launch of any other push carries the touched rows of
// a scan that ran in between, or none).
std::atomic<uint64_t> g_seq{0};
std::atomic<uint64_t> g_prep_seq{0};
std::atomic<int32_t> g_prep_ns{0};

// The launch with the kernel's own start / stop events around it.
template <class F>
hipError_t launch(hipStream_t stream, hipEvent_t start, hipEvent_t stop, F fn) {
  g_seq++;
  if (start)
    if (const hipError_t e = hipEventRecord(start, stream); e != hipSuccess) return e;
  hostsim::enqueue(stream, std::move(fn));
  if (stop) return hipEventRecord(stop, stream);
  return hipSuccess;
}

}  // namespace

// (csrc/kbg_kernels.hip firstfit_geometry: pure host code, the same rule)
FfGeometry firstfit_geometry(int32_t G, bool full_scan) {
  constexpr int kCUs = 256;
  if (!full_scan) {
    const int v = G <= 16 * kCUs ? 16 : G <= 24 * kCUs ? 24 : 32;
    return {v, v};
  }
  int rows = (G + kCUs - 1) / kCUs;
  rows = std::min(32, std::max(2, (rows + 1) & ~1));
  return {rows <= 16 ? 16 : rows <= 24 ? 24 : 32, rows};
}

hipError_t launch_firstfit(const FirstFitArgs& a, int32_t int_mode, hipStream_t stream, hipEvent_t start,
                           hipEvent_t stop) {
  if (a.G <= 0) return hipSuccess;
  const FfGeometry geo = firstfit_geometry(a.G, !a.early_exit);
  if (a.rows <= 0 || a.rows > geo.variant) return hipErrorInvalidValue;
  if (a.complete && a.w_hi - a.w_lo > kFfRoundWords) return hipErrorInvalidValue;
  return launch(stream, start, stop, [a, int_mode] { firstfit_run(a, int_mode != 0); });
}

hipError_t launch_scan(const NodeSoA& n, const ScanGeom& g, const uint64_t* class_mask, const TaskRec* tasks,
                       int32_t n_tasks, int32_t cap_check, int32_t int_mode, uint64_t* out, hipStream_t stream,
                       hipEvent_t start, hipEvent_t stop) {
  if (n_tasks <= 0 || g.n_chunks <= 0) return hipSuccess;
  return launch(stream, start, stop, [n, g, class_mask, tasks, n_tasks, cap_check, int_mode, out] {
    scan_run(n, g, class_mask, tasks, n_tasks, cap_check != 0, int_mode != 0, out);
  });
}

hipError_t launch_select(const uint64_t* bits, int32_t w_lo, int32_t w_hi, int32_t Wl, int32_t n_rows,
                         const uint32_t* cap_off, uint32_t* out_cand, uint32_t* out_count, hipStream_t stream,
                         hipEvent_t start, hipEvent_t stop) {
  if (n_rows <= 0) return hipSuccess;
  return launch(stream, start, stop, [=] { select_run(bits, w_lo, w_hi, Wl, n_rows, cap_off, out_cand, out_count); });
}

hipError_t launch_apply(const NodeSoA& n, const NodeDelta* deltas, int32_t n_deltas, hipStream_t stream) {
  if (n_deltas <= 0) return hipSuccess;
  return launch(stream, nullptr, nullptr, [n, deltas, n_deltas] {
    for (int32_t i = 0; i < n_deltas; ++i) {
      const NodeDelta& d = deltas[i];
      n.idle_cpu[d.node] = d.idle[0];
      n.idle_mem[d.node] = d.idle[1];
      n.idle_gpu[d.node] = d.idle[2];
      n.rel_cpu[d.node] = d.rel[0];
      n.rel_mem[d.node] = d.rel[1];
      n.rel_gpu[d.node] = d.rel[2];
      n.ntasks[d.node] = d.ntasks;
      n.maxtasks[d.node] = d.maxtasks;
    }
  });
}

hipError_t launch_copy16(void* dst, const void* src, size_t n16, hipStream_t stream) {
  if (n16 == 0) return hipSuccess;
  return launch(stream, nullptr, nullptr, [dst, src, n16] { memcpy(dst, src, n16 * 16); });
}

hipError_t launch_mask_apply(uint64_t* class_mask, const MaskDelta* deltas, int32_t n_deltas, hipStream_t stream) {
  if (n_deltas <= 0) return hipSuccess;
  return launch(stream, nullptr, nullptr, [class_mask, deltas, n_deltas] {
    for (int32_t i = 0; i < n_deltas; ++i) class_mask[deltas[i].index] = deltas[i].value;
  });
}

hipError_t launch_fitdelta(const FitArgs& a, hipStream_t stream) {
  if (a.nq <= 0) return hipSuccess;
  return launch(stream, nullptr, nullptr, [a] { fitdelta_run(a); });
}

hipError_t launch_reasons(const ReasonArgs& a, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
  if (a.nq <= 0) return hipSuccess;
  return launch(stream, start, stop, [a] { reasons_run(a); });
}

hipError_t launch_build_class_mask(const StaticTables& t, int32_t n_classes, int32_t W, uint64_t* class_mask,
                                   hipStream_t stream) {
  if (n_classes <= 0 || W <= 0) return hipSuccess;
  return launch(stream, nullptr, nullptr, [t, n_classes, W, class_mask] { class_mask_run(t, n_classes, W, class_mask); });
}

hipError_t launch_build_stage_planes(const StaticTables& t, int32_t n_classes, int32_t W, const StagePlanes& p,
                                     hipStream_t stream) {
  if (n_classes <= 0 || W <= 0) return hipSuccess;
  g_count[kCountStageMask]++;
  return launch(stream, nullptr, nullptr, [t, n_classes, W, p] { stage_planes_run(t, n_classes, W, p); });
}

hipError_t launch_victim_scan(const VictimScan& p, const VictimTables& t, uint32_t* stop_bits, uint32_t* panic_bits,
                              hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
  if (p.node_n <= 0) return hipSuccess;
  g_count[kCountScan]++;
  return launch(stream, start, stop, [p, t, stop_bits, panic_bits] { victim_scan_run(p, t, stop_bits, panic_bits); });
}

hipError_t launch_victim_big(const VictimScan& p, const VictimTables& t, const int32_t* rows, int32_t n_rows,
                             uint32_t* stop_bits, uint32_t* panic_bits, uint8_t* row_out, hipStream_t stream) {
  if (n_rows <= 0) return hipSuccess;
  g_count[row_out ? kCountBigRowOut : kCountBig]++;
  return launch(stream, nullptr, nullptr, [p, t, rows, n_rows, stop_bits, panic_bits, row_out] {
    victim_big_run(p, t, rows, n_rows, stop_bits, panic_bits, row_out);
  });
}

hipError_t launch_victim_prep(const NodeSoA& n, const VictimTables& t, const NodeDelta* nd, int32_t n_nodes,
                              const StateDelta* sd, int32_t n_state, hipStream_t stream) {
  if (n_nodes + n_state <= 0) return hipSuccess;
  g_count[kCountPrep]++;
  if (g_prep_seq.load() == g_seq.load() && g_seq.load() != 0 && (n_nodes > 0 || g_prep_ns.load() == kMaskDeltaCap))
    g_count[kCountPrepNextChunk]++;
  g_prep_ns = n_state;
  const hipError_t e = launch(stream, nullptr, nullptr,
                              [n, t, nd, n_nodes, sd, n_state] { victim_prep_run(n, t, nd, n_nodes, sd, n_state); });
  g_prep_seq = g_seq.load();
  return e;
}

hipError_t launch_victim_prep_inline(const NodeSoA& n, const VictimTables& t, const VictimPrepArgs& a,
                                     hipStream_t stream) {
  if (a.nn + a.ns <= 0) return hipSuccess;
  g_count[kCountPrepInline]++;
  if (a.nn > 0) g_count[kCountPrepInlineNodes]++;
  if (a.ns > 0) g_count[kCountPrepInlineState]++;
  // the deltas travel in the arguments: copied now (an uninitialised tail is not read)
  std::vector<NodeDelta> nd(a.nd, a.nd + a.nn);
  std::vector<StateDelta> sd(a.sd, a.sd + a.ns);
  return launch(stream, nullptr, nullptr, [n, t, nd = std::move(nd), sd = std::move(sd)] {
    victim_prep_run(n, t, nd.data(), (int32_t)nd.size(), sd.data(), (int32_t)sd.size());
  });
}

// (under a counter of its own: the victim counters describe the actions' own launches)
hipError_t launch_victim_why(const VictimWhyArgs& a, const VictimTables& t, hipStream_t stream, hipEvent_t start,
                             hipEvent_t stop) {
  if (a.nq <= 0) return hipSuccess;
  g_count[kCountVictimWhy]++;
  return launch(stream, start, stop, [a, t] { victim_why_run(a, t); });
}

hipError_t launch_victim_why_big(const VictimWhyArgs& a, const VictimTables& t, const int32_t* rows, int32_t n_rows,
                                 hipStream_t stream) {
  if (n_rows <= 0 || a.nq <= 0) return hipSuccess;
  return launch(stream, nullptr, nullptr, [a, t, rows, n_rows] { victim_why_big_run(a, t, rows, n_rows); });
}

hipError_t launch_task_why_init(int32_t* out, int32_t n_shapes, hipStream_t stream) {
  if (n_shapes <= 0) return hipSuccess;
  return launch(stream, nullptr, nullptr, [out, n_shapes] { task_why_init_run(out, n_shapes); });
}

hipError_t launch_task_why(const TaskWhyArgs& a, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
  if (a.n_shapes <= 0 || a.tab_n <= 0) return hipSuccess;
  g_count[kCountTaskWhy]++;
  return launch(stream, start, stop, [a] { task_why_run(a); });
}

hipError_t launch_task_headroom_init(int32_t* out, int32_t n_shapes, hipStream_t stream) {
  if (n_shapes <= 0) return hipSuccess;
  return launch(stream, nullptr, nullptr, [out, n_shapes] { task_headroom_init_run(out, n_shapes); });
}

hipError_t launch_task_headroom(const TaskRoomArgs& a, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
  if (a.limit < 1 || a.limit > kRoomMaxLimit) return hipErrorInvalidValue;
  if ((int64_t)a.tab_n * a.limit > INT32_MAX) return hipErrorInvalidValue;
  if (a.n_shapes <= 0 || a.tab_n <= 0) return hipSuccess;
  g_count[kCountTaskHeadroom]++;
  return launch(stream, start, stop, [a] { task_headroom_run(a); });
}

hipError_t launch_job_fit(const JobFitArgs& a, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
  if (job_fit_refusal(a)) return hipErrorInvalidValue;
  if (a.n_jobs <= 0 || a.tab_n <= 0) return hipSuccess;
  g_count[kCountJobFit]++;
  return launch(stream, start, stop, [a] { job_fit_run(a); });
}

hipError_t launch_drain(const DrainArgs& a, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
  if (drain_refusal(a)) return hipErrorInvalidValue;
  if (a.n_walks <= 0 || a.tab_n <= 0) return hipSuccess;
  g_count[kCountDrain]++;
  return launch(stream, start, stop, [a] { drain_run(a); });
}

hipError_t launch_node_why_init(int32_t* out, int32_t ostride, int32_t n_words, hipStream_t stream) {
  if (n_words <= 0) return hipSuccess;
  if ((int64_t)n_words * 64 > ostride) return hipErrorInvalidValue;
  return launch(stream, nullptr, nullptr, [out, ostride, n_words] { node_why_init_run(out, ostride, n_words); });
}

hipError_t launch_node_why(const NodeWhyArgs& a, hipStream_t stream, hipEvent_t start, hipEvent_t stop) {
  if ((int64_t)a.n_words * 64 > a.ostride) return hipErrorInvalidValue;
  if (a.n_shapes <= 0 || a.tab_n <= 0 || a.n_words <= 0) return hipSuccess;
  g_count[kCountNodeWhy]++;
  return launch(stream, start, stop, [a] { node_why_run(a); });
}

}  // namespace kbg

// The launch counters since the last reset, in the order of
// kbg_hostsim_launch_count_names (comma separated). Exported by
// libkbg_hostsim.so only (tools/hostsim.map); not part of include/kbgpu.h.
extern "C" const char* kbg_hostsim_launch_count_names() { return kbg::kCountNames; }
extern "C" int32_t kbg_hostsim_launch_counts(int64_t* out, int32_t cap) {
  for (int i = 0; i < kbg::kCounts && i < cap; ++i) out[i] = kbg::g_count[i].load();
  return kbg::kCounts;
}
extern "C" void kbg_hostsim_launch_counts_reset() {
  for (auto& c : kbg::g_count) c = 0;
}
