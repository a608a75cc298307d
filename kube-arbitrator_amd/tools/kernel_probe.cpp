// Developer tool (not part of libkbgpu.so): kernel probes. Each entry point
// takes host arrays, allocates what it needs, runs one launcher of
// kbg_device.hpp (or a short chain of them) on a stream of its own,
// synchronises, copies the outputs back and frees everything. There is no
// session and no Grouper: tests/test_kernels_gpu.py builds the inputs and
// compares the raw device output with a plain reference (tests/kernel_ref.py);
// tests/test_victim_kernels_gpu.py does so for the victim scan
// (tests/victim_ref.py), tests/test_victim_why_kernels_gpu.py for the victim
// reasons (tests/victim_why_ref.py), tests/test_task_why_kernels_gpu.py for
// the pending-task reasons (tests/task_why_ref.py),
// tests/test_headroom_kernels_gpu.py for the pending-task headroom
// (tests/headroom_ref.py), tests/test_job_fit_kernels_gpu.py for the job fit
// walk (tests/job_fit_ref.py), tests/test_node_why_kernels_gpu.py for the node
// reasons (tests/node_why_ref.py).
//
// Output buffers are filled with kProbeSentinel bytes before the launch and
// are followed by a guard region of kProbeGuardBytes of the same pattern; the
// whole buffers, guards included, are returned, so a store outside the
// documented range shows. The probes exist to test legal launches: anything
// the session code would never produce is rejected on the host (-2) without
// a launch. Return 0, or a negative code with kbg_tool_probe_error() set.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../csrc/kbg_device.hpp"

namespace {

constexpr int32_t kProbeGuardBytes = 4096;
constexpr int kProbeSentinel = 0xA5;
constexpr int32_t kProbeInvalid = -2, kProbeHip = -3;

thread_local std::string t_error;

int32_t reject(const char* what) {
  t_error = what;
  return kProbeInvalid;
}

// Every allocation of one probe call, freed when it returns.
struct Scope {
  std::vector<void*> dev, host;
  hipStream_t stream = nullptr;
  ~Scope() {
    if (stream) {
      (void)hipStreamSynchronize(stream);
      (void)hipStreamDestroy(stream);
    }
    for (void* p : dev) (void)hipFree(p);
    for (void* p : host) (void)hipHostFree(p);
  }
};

int32_t hip_fail(hipError_t e, const char* what) {
  t_error = std::string(what) + ": " + hipGetErrorString(e);
  return kProbeHip;
}

#define PROBE_TRY(expr)                                  \
  do {                                                   \
    const hipError_t e_ = (expr);                        \
    if (e_ != hipSuccess) return hip_fail(e_, #expr);    \
  } while (0)

// Device memory holding a copy of `src` (or `fill` bytes when src is null).
template <class T>
hipError_t dev_copy(Scope& sc, T** out, const T* src, size_t count, int fill = 0) {
  void* p = nullptr;
  const size_t bytes = std::max<size_t>(count * sizeof(T), 16);
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) return e;
  sc.dev.push_back(p);
  e = src ? hipMemcpy(p, src, count * sizeof(T), hipMemcpyHostToDevice) : hipMemset(p, fill, bytes);
  *out = (T*)p;
  return e;
}

// Host-mapped (zero-copy, coherent) memory as the session's staging uses;
// `dev` is its device address.
template <class T>
hipError_t mapped(Scope& sc, T** host, T** dev, size_t bytes) {
  void* h = nullptr;
  hipError_t e = hipHostMalloc(&h, std::max<size_t>(bytes, 16), hipHostMallocMapped | hipHostMallocCoherent);
  if (e != hipSuccess) return e;
  sc.host.push_back(h);
  void* d = nullptr;
  e = hipHostGetDevicePointer(&d, h, 0);
  *host = (T*)h;
  *dev = (T*)d;
  return e;
}

bool table_ok(int32_t stride, int32_t tab_lo, int32_t tab_n) {
  return stride >= 1 && tab_lo >= 0 && tab_n >= 1 && tab_n <= stride;
}

bool classes_ok(const kbg::TaskRec* t, int32_t n, int32_t classes) {
  for (int32_t i = 0; i < n; ++i)
    if (t[i].cls < 0 || t[i].cls >= classes) return false;
  return true;
}

}  // namespace

extern "C" const char* kbg_tool_probe_error() { return t_error.c_str(); }
extern "C" int32_t kbg_tool_probe_guard_bytes() { return kProbeGuardBytes; }
extern "C" int32_t kbg_tool_probe_sentinel() { return kProbeSentinel; }

// The scalar fields of FirstFitArgs as given, then the probe's own.
struct kbg_probe_ff {
  int32_t G, n_shapes, mw, n_nodes, W, w_lo, w_hi, tab_lo, tab_n, cap_check, early_exit, complete, splits, split_words,
      rows, info_stride, part0, mask_w0, runs;
  int32_t stride;    // rows of the node table block
  int32_t classes;   // rows of class_mask
  int32_t int_mode;
};

// kbg_firstfit_kernel. nodes: the table block (FirstFitArgs.nodes layout,
// stride * 56 bytes); class_mask [classes][W]; shapes [n_shapes]; row_shape
// [G] or null; run_end [n_shapes] (runs != 0) or null. info_out: n_shapes *
// info_stride words + guard; masks_out: n_shapes * mw pairs + guard.
extern "C" int32_t kbg_tool_probe_firstfit(const kbg_probe_ff* p, const void* nodes, const uint64_t* class_mask,
                                           const kbg::TaskRec* shapes, const uint32_t* row_shape,
                                           const uint16_t* run_end, void* info_out, void* masks_out) {
  t_error.clear();
  if (!p || !nodes || !class_mask || !shapes || !info_out || !masks_out) return reject("null argument");
  if (p->G < 1 || p->n_shapes < 1 || p->classes < 1) return reject("empty launch");
  const kbg::FfGeometry geo = kbg::firstfit_geometry(p->G, !p->early_exit);
  if (p->rows < 1 || p->rows > geo.variant) return reject("rows outside 1..geometry.variant");
  if (p->W < 1 || p->w_lo < 0 || p->w_lo >= p->w_hi || p->w_hi > p->W) return reject("w_lo / w_hi outside W");
  const int32_t tw = p->w_hi - p->w_lo;
  if (p->complete && tw > kbg::kFfRoundWords) return reject("complete with more than kFfRoundWords words");
  if (p->n_nodes < 1 || p->n_nodes > p->W * 64) return reject("n_nodes outside W");
  if (!table_ok(p->stride, p->tab_lo, p->tab_n)) return reject("window rows outside the table block");
  if (p->mask_w0 < 0 || p->mask_w0 > p->w_lo || p->mw < p->w_hi - p->mask_w0) return reject("mw too small");
  if (p->splits < 1 || p->splits > kbg::kFfMaxSplits || p->split_words < 1 ||
      (int64_t)p->splits * p->split_words < tw)
    return reject("splits * split_words < w_hi - w_lo");
  if ((int64_t)(p->splits - 1) * p->split_words >= tw) return reject("an empty part");
  if (p->part0 < 0 || p->info_stride < p->part0 + p->splits) return reject("info_stride too small");
  if (!classes_ok(shapes, p->n_shapes, p->classes)) return reject("shape class outside class_mask");
  if (p->runs) {
    if (!run_end || row_shape || p->n_shapes > kbg::kInlineShapes) return reject("runs need inline shapes and run_end");
    uint32_t prev = 0;
    for (int32_t s = 0; s < p->n_shapes; ++s) {
      if (run_end[s] <= prev) return reject("run_end not increasing");
      prev = run_end[s];
    }
    if ((int32_t)prev != p->G) return reject("run_end does not add up to G");
  } else if (row_shape) {
    std::vector<int> writers(p->n_shapes, 0);
    for (int32_t g = 0; g < p->G; ++g) {
      const uint32_t s = row_shape[g] & ~kbg::kRowWriter;
      if (s >= (uint32_t)p->n_shapes) return reject("row_shape outside the shape table");
      if (row_shape[g] & kbg::kRowWriter) writers[s]++;
    }
    for (int w : writers)
      if (w > 1) return reject("two writer rows of one shape");
  } else if (p->G > p->n_shapes) {
    return reject("G > n_shapes without a row map");
  }

  Scope sc;
  PROBE_TRY(hipStreamCreate(&sc.stream));
  kbg::FirstFitArgs a{};
  double* d_nodes = nullptr;
  PROBE_TRY(dev_copy(sc, (char**)&d_nodes, (const char*)nodes, (size_t)p->stride * 56));
  uint64_t* d_cm = nullptr;
  PROBE_TRY(dev_copy(sc, &d_cm, class_mask, (size_t)p->classes * p->W));
  a.nodes = d_nodes;
  a.class_mask = d_cm;
  if (p->n_shapes <= kbg::kInlineShapes) {
    std::copy(shapes, shapes + p->n_shapes, a.inl);
  } else {  // host-mapped, as device_launch does
    kbg::TaskRec *h = nullptr, *d = nullptr;
    PROBE_TRY(mapped(sc, &h, &d, (size_t)p->n_shapes * sizeof(kbg::TaskRec)));
    std::copy(shapes, shapes + p->n_shapes, h);
    a.shapes = d;
  }
  if (p->runs) {
    std::copy(run_end, run_end + p->n_shapes, a.run_end);
  } else if (row_shape) {
    uint32_t *h = nullptr, *d = nullptr;
    PROBE_TRY(mapped(sc, &h, &d, (size_t)p->G * 4));
    std::copy(row_shape, row_shape + p->G, h);
    a.row_shape = d;
  }
  const size_t info_bytes = (size_t)p->n_shapes * p->info_stride * 4 + kProbeGuardBytes;
  const size_t mask_bytes = (size_t)p->n_shapes * p->mw * sizeof(kbg::MaskPair) + kProbeGuardBytes;
  char *h_info = nullptr, *h_masks = nullptr;
  PROBE_TRY(mapped(sc, &h_info, (char**)&a.info, info_bytes));
  PROBE_TRY(mapped(sc, &h_masks, (char**)&a.masks, mask_bytes));
  memset(h_info, kProbeSentinel, info_bytes);
  memset(h_masks, kProbeSentinel, mask_bytes);
  a.avail = nullptr;
  a.stride = p->stride;
  a.G = p->G;
  a.n_shapes = p->n_shapes;
  a.mw = p->mw;
  a.n_nodes = p->n_nodes;
  a.W = p->W;
  a.w_lo = p->w_lo;
  a.w_hi = p->w_hi;
  a.tab_lo = p->tab_lo;
  a.tab_n = p->tab_n;
  a.cap_check = p->cap_check;
  a.early_exit = p->early_exit;
  a.complete = p->complete;
  a.splits = p->splits;
  a.split_words = p->split_words;
  a.rows = p->rows;
  a.info_stride = p->info_stride;
  a.part0 = p->part0;
  a.mask_w0 = p->mask_w0;
  a.runs = p->runs;
  PROBE_TRY(kbg::launch_firstfit(a, p->int_mode ? 1 : 0, sc.stream));
  PROBE_TRY(hipStreamSynchronize(sc.stream));
  memcpy(info_out, h_info, info_bytes);
  memcpy(masks_out, h_masks, mask_bytes);
  return 0;
}

struct kbg_probe_scan {
  int32_t n_nodes, W, Wl, slots, tab_lo, stride, classes, n_tasks, cap_check, int_mode, w_lo, w_hi;
};

// kbg_scan_kernel, one launch per slot as a rank of a sharded session scans
// its own, into one [slot][plane][quad][row][4] buffer, then
// kbg_select_kernel over [w_lo, w_hi). tasks [n_tasks] (padded here as
// kbg_pad_rows asks); cap_off [n_tasks + 1]. bits_out: slots * 2 * n_tasks *
// kbg_slot_words(Wl) words + guard; cand_out: cap_off[n_tasks] words + guard;
// count_out: n_tasks words + guard.
extern "C" int32_t kbg_tool_probe_scan_select(const kbg_probe_scan* p, const void* nodes, const uint64_t* class_mask,
                                              const kbg::TaskRec* tasks, const uint32_t* cap_off, void* bits_out,
                                              void* cand_out, void* count_out) {
  t_error.clear();
  if (!p || !nodes || !class_mask || !tasks || !cap_off || !bits_out || !cand_out || !count_out)
    return reject("null argument");
  if (p->n_tasks < 1 || p->classes < 1 || p->Wl < 1 || p->slots < 1) return reject("empty launch");
  if (p->W < 1 || p->n_nodes < 1 || p->n_nodes > p->W * 64 || (int64_t)p->slots * p->Wl < p->W)
    return reject("slots do not cover W");
  if ((int64_t)(p->slots - 1) * p->Wl >= p->W) return reject("a slot past W");
  if (p->w_lo < 0 || p->w_lo > p->w_hi || p->w_hi > p->W) return reject("w_lo / w_hi outside W");
  // the scan kernel reads the row of every node below n_nodes
  if (p->stride < 1 || p->tab_lo != 0 || p->n_nodes > p->stride) return reject("nodes outside the table block");
  if (!classes_ok(tasks, p->n_tasks, p->classes)) return reject("task class outside class_mask");
  for (int32_t t = 0; t < p->n_tasks; ++t)
    if (cap_off[t + 1] < cap_off[t]) return reject("cap_off not increasing");
  if (cap_off[0] != 0) return reject("cap_off[0] != 0");

  Scope sc;
  PROBE_TRY(hipStreamCreate(&sc.stream));
  double* d = nullptr;
  const size_t L = (size_t)p->stride;
  PROBE_TRY(dev_copy(sc, (char**)&d, (const char*)nodes, L * 56));
  const kbg::NodeSoA soa{d, d + L, d + 2 * L, d + 3 * L, d + 4 * L, d + 5 * L, (int32_t*)(d + 6 * L),
                         (int32_t*)(d + 6 * L) + L};
  uint64_t* d_cm = nullptr;
  PROBE_TRY(dev_copy(sc, &d_cm, class_mask, (size_t)p->classes * p->W));
  std::vector<kbg::TaskRec> rows(tasks, tasks + p->n_tasks);
  rows.resize(kbg::kbg_pad_rows(p->n_tasks), tasks[0]);  // padding rows: scanned, never stored
  kbg::TaskRec* d_tasks = nullptr;
  PROBE_TRY(dev_copy(sc, &d_tasks, rows.data(), rows.size()));
  uint32_t* d_capoff = nullptr;
  PROBE_TRY(dev_copy(sc, &d_capoff, cap_off, (size_t)p->n_tasks + 1));
  const size_t slot_words = (size_t)2 * p->n_tasks * kbg::kbg_slot_words(p->Wl);
  const size_t bits_bytes = (size_t)p->slots * slot_words * 8 + kProbeGuardBytes;
  const size_t cand_bytes = (size_t)cap_off[p->n_tasks] * 4 + kProbeGuardBytes;
  const size_t count_bytes = (size_t)p->n_tasks * 4 + kProbeGuardBytes;
  char *d_bits = nullptr, *d_cand = nullptr, *d_count = nullptr;
  PROBE_TRY(dev_copy(sc, &d_bits, (const char*)nullptr, bits_bytes, kProbeSentinel));
  PROBE_TRY(dev_copy(sc, &d_cand, (const char*)nullptr, cand_bytes, kProbeSentinel));
  PROBE_TRY(dev_copy(sc, &d_count, (const char*)nullptr, count_bytes, kProbeSentinel));
  for (int32_t s = 0; s < p->slots; ++s) {
    const kbg::ScanGeom geo{p->n_nodes, p->W, p->Wl, s * p->Wl, p->Wl, p->tab_lo};
    PROBE_TRY(kbg::launch_scan(soa, geo, d_cm, d_tasks, p->n_tasks, p->cap_check, p->int_mode ? 1 : 0,
                               (uint64_t*)d_bits + (size_t)s * slot_words, sc.stream));
  }
  PROBE_TRY(hipStreamSynchronize(sc.stream));
  PROBE_TRY(hipMemcpy(bits_out, d_bits, bits_bytes, hipMemcpyDeviceToHost));
  // The select kernel reads only the words [w_lo, w_hi) <= W the scans wrote.
  PROBE_TRY(kbg::launch_select((const uint64_t*)d_bits, p->w_lo, p->w_hi, p->Wl, p->n_tasks, d_capoff,
                               (uint32_t*)d_cand, (uint32_t*)d_count, sc.stream));
  PROBE_TRY(hipStreamSynchronize(sc.stream));
  PROBE_TRY(hipMemcpy(cand_out, d_cand, cand_bytes, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(count_out, d_count, count_bytes, hipMemcpyDeviceToHost));
  return 0;
}

struct kbg_probe_fit {
  int32_t n_nodes, W, stride, classes, tab_lo, tab_n, nq, cap_check, n_dec;
};

// kbg_fitdelta_kernel. hoff [n_nodes + 1] (global nodes); hk, na [n_dec];
// hold [n_dec][3]; q [nq]. out: nq * 4 words + guard (host-mapped).
extern "C" int32_t kbg_tool_probe_fitdelta(const kbg_probe_fit* p, const void* nodes, const uint64_t* class_mask,
                                           const int32_t* hoff, const int32_t* hk, const double* hold,
                                           const int32_t* na, const kbg::FitQuery* q, void* out) {
  t_error.clear();
  if (!p || !nodes || !class_mask || !hoff || !hk || !hold || !na || !q || !out) return reject("null argument");
  if (p->nq < 1 || p->classes < 1) return reject("empty launch");
  if (p->n_nodes < 1 || p->W < 1 || p->n_nodes > p->W * 64) return reject("n_nodes outside W");
  if (!table_ok(p->stride, p->tab_lo, p->tab_n) || p->tab_lo + p->tab_n > p->n_nodes)
    return reject("window rows outside the table block");
  if (hoff[0] != 0 || hoff[p->n_nodes] != p->n_dec) return reject("hoff does not span the decisions");
  for (int32_t n = 0; n < p->n_nodes; ++n)
    if (hoff[n + 1] < hoff[n]) return reject("hoff not increasing");
  for (int32_t i = 0; i < p->n_dec; ++i)
    if (na[i] < -1 || na[i] >= p->n_dec) return reject("na outside the decisions");
  for (int32_t i = 0; i < p->nq; ++i)
    if (q[i].cls < 0 || q[i].cls >= p->classes || q[i].end < 0) return reject("query outside class_mask");

  Scope sc;
  PROBE_TRY(hipStreamCreate(&sc.stream));
  kbg::FitArgs a{};
  PROBE_TRY(dev_copy(sc, (char**)&a.nodes, (const char*)nodes, (size_t)p->stride * 56));
  PROBE_TRY(dev_copy(sc, (uint64_t**)&a.class_mask, class_mask, (size_t)p->classes * p->W));
  PROBE_TRY(dev_copy(sc, (int32_t**)&a.hoff, hoff, (size_t)p->n_nodes + 1));
  PROBE_TRY(dev_copy(sc, (int32_t**)&a.hk, hk, (size_t)p->n_dec));
  PROBE_TRY(dev_copy(sc, (double**)&a.hold, hold, (size_t)p->n_dec * 3));
  PROBE_TRY(dev_copy(sc, (int32_t**)&a.na, na, (size_t)p->n_dec));
  PROBE_TRY(dev_copy(sc, (kbg::FitQuery**)&a.q, q, (size_t)p->nq));
  a.stride = p->stride;
  a.W = p->W;
  a.nq = p->nq;
  a.cap_check = p->cap_check;
  a.tab_lo = p->tab_lo;
  a.tab_n = p->tab_n;
  const size_t out_bytes = (size_t)p->nq * 16 + kProbeGuardBytes;
  char* h_out = nullptr;
  PROBE_TRY(mapped(sc, &h_out, (char**)&a.out, out_bytes));
  memset(h_out, kProbeSentinel, out_bytes);
  PROBE_TRY(kbg::launch_fitdelta(a, sc.stream));
  PROBE_TRY(hipStreamSynchronize(sc.stream));
  memcpy(out, h_out, out_bytes);
  return 0;
}

// kbg_apply_kernel on the table, kbg_mask_apply_kernel on the mask words,
// then kbg_copy16_kernel of the table into a second buffer. `nodes`
// (stride * 56 bytes, stride even: whole 16-byte units) and `mask`
// [mask_words] are updated in place; copy_out: stride * 56 bytes + guard.
extern "C" int32_t kbg_tool_probe_apply(int32_t stride, void* nodes, const kbg::NodeDelta* deltas, int32_t n_deltas,
                                        uint64_t* mask, int32_t mask_words, const kbg::MaskDelta* mdeltas,
                                        int32_t n_mdeltas, void* copy_out) {
  t_error.clear();
  if (!nodes || !deltas || !mask || !mdeltas || !copy_out) return reject("null argument");
  if (stride < 2 || (stride & 1) || mask_words < 1 || n_deltas < 1 || n_mdeltas < 1) return reject("empty launch");
  for (int32_t i = 0; i < n_deltas; ++i)
    if (deltas[i].node < 0 || deltas[i].node >= stride) return reject("delta outside the table");
  for (int32_t i = 0; i < n_mdeltas; ++i)
    if (mdeltas[i].index >= (uint32_t)mask_words) return reject("mask delta outside the mask");

  Scope sc;
  PROBE_TRY(hipStreamCreate(&sc.stream));
  const size_t L = (size_t)stride, bytes = L * 56;
  double* d = nullptr;
  PROBE_TRY(dev_copy(sc, (char**)&d, (const char*)nodes, bytes));
  const kbg::NodeSoA soa{d, d + L, d + 2 * L, d + 3 * L, d + 4 * L, d + 5 * L, (int32_t*)(d + 6 * L),
                         (int32_t*)(d + 6 * L) + L};
  uint64_t* d_mask = nullptr;
  PROBE_TRY(dev_copy(sc, &d_mask, mask, (size_t)mask_words));
  // deltas are read in place from host-mapped memory, as the session's are
  kbg::NodeDelta *h_nd = nullptr, *d_nd = nullptr;
  PROBE_TRY(mapped(sc, &h_nd, &d_nd, (size_t)n_deltas * sizeof(kbg::NodeDelta)));
  std::copy(deltas, deltas + n_deltas, h_nd);
  kbg::MaskDelta *h_md = nullptr, *d_md = nullptr;
  PROBE_TRY(mapped(sc, &h_md, &d_md, (size_t)n_mdeltas * sizeof(kbg::MaskDelta)));
  std::copy(mdeltas, mdeltas + n_mdeltas, h_md);
  char* d_copy = nullptr;
  PROBE_TRY(dev_copy(sc, &d_copy, (const char*)nullptr, bytes + kProbeGuardBytes, kProbeSentinel));
  PROBE_TRY(kbg::launch_apply(soa, d_nd, n_deltas, sc.stream));
  PROBE_TRY(kbg::launch_mask_apply(d_mask, d_md, n_mdeltas, sc.stream));
  PROBE_TRY(kbg::launch_copy16(d_copy, d, bytes / 16, sc.stream));
  PROBE_TRY(hipStreamSynchronize(sc.stream));
  PROBE_TRY(hipMemcpy(nodes, d, bytes, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(mask, d_mask, (size_t)mask_words * 8, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(copy_out, d_copy, bytes + kProbeGuardBytes, hipMemcpyDeviceToHost));
  return 0;
}

struct kbg_probe_stage {
  int32_t n_nodes, W, classes, label_words, taint_words, n_numcols, n_reqs, n_terms, mask_pool_words, tol_pool_words;
};

// kbg_stage_mask_kernel, and kbg_mask_kernel on the same tables. label_bits
// [label_words][n_nodes], taint_bits [taint_words][n_nodes], num_vals, num_ok
// [n_numcols][n_nodes], name_id, node_flags [n_nodes], the pools, reqs
// [n_reqs], terms [n_terms], progs [classes]. planes_out: sel_ok, taint_ok
// [classes][W], unsched, live [W] (kbg_stage_planes) + guard; mask_out:
// [classes][W] + guard.
extern "C" int32_t kbg_tool_probe_stage_mask(const kbg_probe_stage* p, const uint64_t* label_bits,
                                             const uint64_t* taint_bits, const int64_t* num_vals, const uint8_t* num_ok,
                                             const int32_t* name_id, const uint8_t* node_flags,
                                             const uint64_t* mask_pool, const uint64_t* tol_pool,
                                             const kbg::ReqProg* reqs, const kbg::TermProg* terms,
                                             const kbg::ClassProg* progs, void* planes_out, void* mask_out) {
  t_error.clear();
  if (!p || !label_bits || !taint_bits || !num_vals || !num_ok || !name_id || !node_flags || !mask_pool || !tol_pool ||
      !reqs || !terms || !progs || !planes_out || !mask_out)
    return reject("null argument");
  if (p->classes < 1 || p->n_nodes < 1 || p->W < 1 || p->n_nodes > p->W * 64) return reject("n_nodes outside W");
  if (p->label_words < 0 || p->taint_words < 0 || p->n_numcols < 0 || p->n_reqs < 0 || p->n_terms < 0)
    return reject("negative count");
  for (int32_t i = 0; i < p->n_reqs; ++i) {
    const kbg::ReqProg& r = reqs[i];
    if (r.kind < kbg::REQ_FALSE || r.kind > kbg::REQ_NAME_NE) return reject("requirement kind");
    if (r.kind >= kbg::REQ_ALL && r.kind <= kbg::REQ_NONE &&
        (r.mask_off < 0 || r.mask_off + p->label_words > p->mask_pool_words))
      return reject("requirement mask outside the pool");
    if ((r.kind == kbg::REQ_GT || r.kind == kbg::REQ_LT) && (r.col < 0 || r.col >= p->n_numcols))
      return reject("requirement column");
  }
  for (int32_t i = 0; i < p->n_terms; ++i)
    if (terms[i].req_off < 0 || terms[i].req_len < 0 || terms[i].req_off + terms[i].req_len > p->n_reqs)
      return reject("term outside the requirements");
  for (int32_t c = 0; c < p->classes; ++c) {
    const kbg::ClassProg& k = progs[c];
    if (k.sel_req >= p->n_reqs) return reject("class selector outside the requirements");
    if (k.has_affinity && (k.term_off < 0 || k.term_len < 0 || k.term_off + k.term_len > p->n_terms))
      return reject("class terms outside the terms");
    if (k.tol_off < 0 || k.tol_off + p->taint_words > p->tol_pool_words) return reject("class tolerations outside the pool");
  }

  Scope sc;
  PROBE_TRY(hipStreamCreate(&sc.stream));
  const size_t N = (size_t)p->n_nodes;
  kbg::StaticTables t{};
  t.n_nodes = p->n_nodes;
  t.label_words = p->label_words;
  t.taint_words = p->taint_words;
  t.n_numcols = p->n_numcols;
  PROBE_TRY(dev_copy(sc, (uint64_t**)&t.label_bits, label_bits, (size_t)p->label_words * N));
  PROBE_TRY(dev_copy(sc, (uint64_t**)&t.taint_bits, taint_bits, (size_t)p->taint_words * N));
  PROBE_TRY(dev_copy(sc, (int64_t**)&t.num_vals, num_vals, (size_t)p->n_numcols * N));
  PROBE_TRY(dev_copy(sc, (uint8_t**)&t.num_ok, num_ok, (size_t)p->n_numcols * N));
  PROBE_TRY(dev_copy(sc, (int32_t**)&t.name_id, name_id, N));
  PROBE_TRY(dev_copy(sc, (uint8_t**)&t.node_flags, node_flags, N));
  PROBE_TRY(dev_copy(sc, (uint64_t**)&t.mask_pool, mask_pool, (size_t)p->mask_pool_words));
  PROBE_TRY(dev_copy(sc, (uint64_t**)&t.tol_pool, tol_pool, (size_t)p->tol_pool_words));
  PROBE_TRY(dev_copy(sc, (kbg::ReqProg**)&t.reqs, reqs, (size_t)p->n_reqs));
  PROBE_TRY(dev_copy(sc, (kbg::TermProg**)&t.terms, terms, (size_t)p->n_terms));
  PROBE_TRY(dev_copy(sc, (kbg::ClassProg**)&t.classes, progs, (size_t)p->classes));
  const size_t plane_bytes = kbg::kbg_stage_words(p->classes, p->W) * 8 + kProbeGuardBytes;
  const size_t mask_bytes = (size_t)p->classes * p->W * 8 + kProbeGuardBytes;
  char *d_planes = nullptr, *d_mask = nullptr;
  PROBE_TRY(dev_copy(sc, &d_planes, (const char*)nullptr, plane_bytes, kProbeSentinel));
  PROBE_TRY(dev_copy(sc, &d_mask, (const char*)nullptr, mask_bytes, kProbeSentinel));
  PROBE_TRY(kbg::launch_build_stage_planes(t, p->classes, p->W, kbg::kbg_stage_planes((uint64_t*)d_planes, p->classes, p->W),
                                           sc.stream));
  PROBE_TRY(kbg::launch_build_class_mask(t, p->classes, p->W, (uint64_t*)d_mask, sc.stream));
  PROBE_TRY(hipStreamSynchronize(sc.stream));
  PROBE_TRY(hipMemcpy(planes_out, d_planes, plane_bytes, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(mask_out, d_mask, mask_bytes, hipMemcpyDeviceToHost));
  return 0;
}

// kbg_reasons_kernel on kbg_fitdelta_kernel's staging (kbg_probe_fit; hold and
// na are not read). planes: sel_ok, taint_ok [classes][W], unsched, live [W].
// out: nq * kReasonOut words + guard (host-mapped).
extern "C" int32_t kbg_tool_probe_reasons(const kbg_probe_fit* p, const void* nodes, const uint64_t* planes,
                                          const int32_t* hoff, const int32_t* hk, const kbg::FitQuery* q, void* out) {
  t_error.clear();
  if (!p || !nodes || !planes || !hoff || !hk || !q || !out) return reject("null argument");
  if (p->nq < 1 || p->classes < 1) return reject("empty launch");
  if (p->n_nodes < 1 || p->W < 1 || p->n_nodes > p->W * 64) return reject("n_nodes outside W");
  if (!table_ok(p->stride, p->tab_lo, p->tab_n) || p->tab_lo + p->tab_n > p->n_nodes)
    return reject("window rows outside the table block");
  if (hoff[0] != 0 || hoff[p->n_nodes] != p->n_dec) return reject("hoff does not span the decisions");
  for (int32_t n = 0; n < p->n_nodes; ++n)
    if (hoff[n + 1] < hoff[n]) return reject("hoff not increasing");
  for (int32_t i = 0; i < p->nq; ++i)
    if (q[i].cls < 0 || q[i].cls >= p->classes || q[i].end < 0 || q[i].end > p->n_nodes || q[i].win < -1 ||
        q[i].win >= p->n_nodes)
      return reject("query outside the planes");

  Scope sc;
  PROBE_TRY(hipStreamCreate(&sc.stream));
  kbg::ReasonArgs a{};
  uint64_t* d_planes = nullptr;
  PROBE_TRY(dev_copy(sc, (char**)&a.nodes, (const char*)nodes, (size_t)p->stride * 56));
  PROBE_TRY(dev_copy(sc, &d_planes, planes, kbg::kbg_stage_words(p->classes, p->W)));
  PROBE_TRY(dev_copy(sc, (int32_t**)&a.hoff, hoff, (size_t)p->n_nodes + 1));
  PROBE_TRY(dev_copy(sc, (int32_t**)&a.hk, hk, (size_t)p->n_dec));
  PROBE_TRY(dev_copy(sc, (kbg::FitQuery**)&a.q, q, (size_t)p->nq));
  const kbg::StagePlanes sp = kbg::kbg_stage_planes(d_planes, p->classes, p->W);
  a.sel_ok = sp.sel_ok;
  a.taint_ok = sp.taint_ok;
  a.unsched = sp.unsched;
  a.live = sp.live;
  a.stride = p->stride;
  a.W = p->W;
  a.nq = p->nq;
  a.cap_check = p->cap_check;
  a.tab_lo = p->tab_lo;
  a.tab_n = p->tab_n;
  const size_t out_bytes = (size_t)p->nq * kbg::kReasonOut * 4 + kProbeGuardBytes;
  char* h_out = nullptr;
  PROBE_TRY(mapped(sc, &h_out, (char**)&a.out, out_bytes));
  memset(h_out, kProbeSentinel, out_bytes);
  PROBE_TRY(kbg::launch_reasons(a, sc.stream));
  PROBE_TRY(hipStreamSynchronize(sc.stream));
  memcpy(out, h_out, out_bytes);
  return 0;
}

// The scalar fields of VictimScan (the deciding tier's fns in tier_fns, as the
// session passes one tier at most), then the probe's own.
struct kbg_probe_victim {
  int32_t n_nodes, W, cls, cap_check, node_lo, node_n, mode, n_tiers, tier_fns, job, queue;
  int32_t stride;    // rows of the node table block (row = node - node_lo)
  int32_t classes;   // rows of class_mask
  int32_t n_cand, n_jobs, n_queues;
  int32_t prep;      // 0 none, 1 launch_victim_prep_inline, 2 launch_victim_prep (host-mapped deltas)
  int32_t nn, ns;    // node deltas, state deltas
  int32_t out_mode;  // 0 mapped (host-mapped words, row_out bytes), 1 device (device words, atomicOr)
  int32_t n_rows;    // the caller's count of big rows (sizes row_out); checked against the probe's own
};

// What try_task runs for one preemptor: an optional prep, kbg_victim_kernel,
// then kbg_victim_big_kernel over the rows of [node_lo, node_lo + node_n)
// holding 129..kMaxNodeCandidates candidates (vt_setup's rule). nodes: the
// table block (stride * 56 bytes), updated in place by the prep, as are c_run
// [n_cand], j_ready [n_jobs], j_alloc [n_jobs][3], q_alloc [n_queues][3].
// dbl: req[3], ls, drf_total[3]. stop, panic: kbg_victim_words(n_nodes) words
// + guard each, in and out (the caller supplies their initial content);
// row_out: n_rows bytes + guard, written in mapped mode only.
extern "C" int32_t kbg_tool_probe_victim(const kbg_probe_victim* p, void* nodes, const uint8_t* panic_node,
                                         const uint64_t* class_mask, const int32_t* nt_off, const int32_t* c_jq,
                                         const double* c_req, uint8_t* c_run, const int32_t* j_min, int32_t* j_ready,
                                         double* j_alloc, double* q_alloc, const double* q_deserved, const double* dbl,
                                         const kbg::NodeDelta* nd, const kbg::StateDelta* sd, void* stop, void* panic,
                                         void* row_out) {
  t_error.clear();
  if (!p || !nodes || !panic_node || !class_mask || !nt_off || !c_jq || !c_req || !c_run || !j_min || !j_ready ||
      !j_alloc || !q_alloc || !q_deserved || !dbl || !nd || !sd || !stop || !panic || !row_out)
    return reject("null argument");
  if (p->n_nodes < 1 || p->W < 1 || p->n_nodes > p->W * 64) return reject("n_nodes outside W");
  if (p->node_lo < 0 || (p->node_lo & 63)) return reject("node_lo not a multiple of 64");
  if (p->node_n < 1 || (int64_t)p->node_lo + p->node_n > p->n_nodes) return reject("node range outside n_nodes");
  if (p->stride < 1 || p->node_n > p->stride) return reject("node range outside the table block");
  if (p->classes < 1 || p->cls < 0 || p->cls >= p->classes) return reject("cls outside class_mask");
  if (p->mode < kbg::VM_PREEMPT_JOBS || p->mode > kbg::VM_RECLAIM) return reject("mode outside 0..2");
  if (p->n_tiers < 0 || p->n_tiers > 1) return reject("n_tiers outside {0, 1}");
  if (p->tier_fns & ~(kbg::VP_GANG | kbg::VP_DRF | kbg::VP_PROP)) return reject("tier_fns outside the victim fns");
  if (p->n_tiers == 1 && p->tier_fns == 0) return reject("tier_fns: a tier without a victim fn");
  if (p->n_cand < 0 || p->n_jobs < 1 || p->n_queues < 1) return reject("empty tables");
  if (p->job < 0 || p->job >= p->n_jobs || p->queue < 0 || p->queue >= p->n_queues)
    return reject("preemptor job or queue outside its table");
  if (nt_off[0] != 0 || nt_off[p->n_nodes] != p->n_cand) return reject("nt_off does not span the candidates");
  for (int32_t n = 0; n < p->n_nodes; ++n)
    if (nt_off[n + 1] < nt_off[n]) return reject("nt_off not increasing");
  for (int32_t k = 0; k < p->n_cand; ++k)
    if (c_jq[2 * k] < 0 || c_jq[2 * k] >= p->n_jobs || c_jq[2 * k + 1] < 0 || c_jq[2 * k + 1] >= p->n_queues)
      return reject("candidate job or queue outside its table");
  if (p->prep < 0 || p->prep > 2 || p->nn < 0 || p->ns < 0) return reject("prep outside 0..2");
  if (p->prep == 0 && p->nn + p->ns != 0) return reject("prep: deltas without a prep launch");
  if (p->prep == 1 && (p->nn > kbg::kArgNodeDeltas || p->ns > kbg::kArgStateDeltas))
    return reject("prep: more deltas than the inline arguments hold");
  if (p->ns > kbg::kMaskDeltaCap) return reject("prep: more state deltas than one staging holds");
  {
    std::vector<char> seen_row(p->stride, 0);
    for (int32_t i = 0; i < p->nn; ++i) {
      if (nd[i].node < 0 || nd[i].node >= p->stride) return reject("delta: node row outside the table block");
      if (seen_row[nd[i].node]++) return reject("delta: duplicate node row");
    }
    const int32_t sizes[4] = {p->n_cand, p->n_jobs, p->n_jobs, p->n_queues};
    std::vector<char> seen[4];
    for (int k = 0; k < 4; ++k) seen[k].assign(std::max(sizes[k], 1), 0);
    for (int32_t i = 0; i < p->ns; ++i) {
      if (sd[i].kind < 0 || sd[i].kind > 3) return reject("delta: kind outside 0..3");
      if (sd[i].index < 0 || sd[i].index >= sizes[sd[i].kind]) return reject("delta: index outside its table");
      if (seen[sd[i].kind][sd[i].index]++) return reject("delta: duplicate (kind, index)");
    }
  }
  // nodes of the range for kbg_victim_big_kernel, as vt_setup lists them
  std::vector<int32_t> big_rows;
  for (int32_t n = p->node_lo; n < p->node_lo + p->node_n; ++n) {
    const int32_t L = nt_off[n + 1] - nt_off[n];
    if (L > 128 && L <= kbg::kMaxNodeCandidates) big_rows.push_back(n - p->node_lo);
  }
  if (p->n_rows != (int32_t)big_rows.size()) return reject("n_rows is not the number of big rows");
  if (p->out_mode < 0 || p->out_mode > 1) return reject("out_mode outside 0..1");

  Scope sc;
  PROBE_TRY(hipStreamCreate(&sc.stream));
  const size_t L = (size_t)p->stride, P = (size_t)p->n_cand, J = (size_t)p->n_jobs, Q = (size_t)p->n_queues;
  double* d = nullptr;
  PROBE_TRY(dev_copy(sc, (char**)&d, (const char*)nodes, L * 56));
  const kbg::NodeSoA soa{d, d + L, d + 2 * L, d + 3 * L, d + 4 * L, d + 5 * L, (int32_t*)(d + 6 * L),
                         (int32_t*)(d + 6 * L) + L};
  kbg::VictimTables t{};
  t.ntasks = soa.ntasks;
  t.maxtasks = soa.maxtasks;
  PROBE_TRY(dev_copy(sc, (uint8_t**)&t.panic_node, panic_node, (size_t)p->n_nodes));
  PROBE_TRY(dev_copy(sc, (uint64_t**)&t.class_mask, class_mask, (size_t)p->classes * p->W));
  PROBE_TRY(dev_copy(sc, (int32_t**)&t.nt_off, nt_off, (size_t)p->n_nodes + 1));
  PROBE_TRY(dev_copy(sc, (int32_t**)&t.c_jq, c_jq, 2 * P));
  PROBE_TRY(dev_copy(sc, (double**)&t.c_req, c_req, 3 * P));
  PROBE_TRY(dev_copy(sc, &t.c_run, (const uint8_t*)c_run, P));
  PROBE_TRY(dev_copy(sc, (int32_t**)&t.j_queue, (const int32_t*)nullptr, J));  // not read by the kernels
  PROBE_TRY(dev_copy(sc, (int32_t**)&t.j_min, j_min, J));
  PROBE_TRY(dev_copy(sc, &t.j_ready, (const int32_t*)j_ready, J));
  PROBE_TRY(dev_copy(sc, &t.j_alloc, (const double*)j_alloc, 3 * J));
  PROBE_TRY(dev_copy(sc, &t.q_alloc, (const double*)q_alloc, 3 * Q));
  PROBE_TRY(dev_copy(sc, (double**)&t.q_deserved, q_deserved, 3 * Q));
  std::copy(dbl + 4, dbl + 7, t.drf_total);
  int32_t* d_rows = nullptr;
  PROBE_TRY(dev_copy(sc, &d_rows, big_rows.data(), big_rows.size()));

  kbg::VictimScan a{};
  a.n_nodes = p->n_nodes;
  a.W = p->W;
  a.cls = p->cls;
  a.cap_check = p->cap_check;
  a.node_lo = p->node_lo;
  a.node_n = p->node_n;
  a.mode = p->mode;
  a.n_tiers = p->n_tiers;
  a.tier_fns[0] = p->tier_fns;
  a.job = p->job;
  a.queue = p->queue;
  std::copy(dbl, dbl + 3, a.req);
  a.ls = dbl[3];

  const size_t word_bytes = (size_t)kbg::kbg_victim_words(p->n_nodes) * 4 + kProbeGuardBytes;
  const size_t row_bytes = big_rows.size() + kProbeGuardBytes;
  char *h_stop = nullptr, *h_panic = nullptr, *h_rows = nullptr;
  uint32_t *d_stop = nullptr, *d_panic = nullptr;
  uint8_t* d_row_out = nullptr;
  if (p->out_mode == 0) {
    PROBE_TRY(mapped(sc, &h_stop, (char**)&d_stop, word_bytes));
    PROBE_TRY(mapped(sc, &h_panic, (char**)&d_panic, word_bytes));
    PROBE_TRY(mapped(sc, &h_rows, (char**)&d_row_out, row_bytes));
    memcpy(h_stop, stop, word_bytes);
    memcpy(h_panic, panic, word_bytes);
    memset(h_rows, kProbeSentinel, row_bytes);
  } else {
    PROBE_TRY(dev_copy(sc, (char**)&d_stop, (const char*)stop, word_bytes));
    PROBE_TRY(dev_copy(sc, (char**)&d_panic, (const char*)panic, word_bytes));
  }

  if (p->prep == 1) {
    kbg::VictimPrepArgs pa{};
    pa.nn = p->nn;
    pa.ns = p->ns;
    std::copy(nd, nd + p->nn, pa.nd);
    std::copy(sd, sd + p->ns, pa.sd);
    PROBE_TRY(kbg::launch_victim_prep_inline(soa, t, pa, sc.stream));
  } else if (p->prep == 2) {  // read in place from host-mapped memory, as the session's staging is
    kbg::NodeDelta *h_nd = nullptr, *d_nd = nullptr;
    kbg::StateDelta *h_sd = nullptr, *d_sd = nullptr;
    PROBE_TRY(mapped(sc, &h_nd, &d_nd, (size_t)p->nn * sizeof(kbg::NodeDelta)));
    PROBE_TRY(mapped(sc, &h_sd, &d_sd, (size_t)p->ns * sizeof(kbg::StateDelta)));
    std::copy(nd, nd + p->nn, h_nd);
    std::copy(sd, sd + p->ns, h_sd);
    PROBE_TRY(kbg::launch_victim_prep(soa, t, d_nd, p->nn, d_sd, p->ns, sc.stream));
  }
  PROBE_TRY(kbg::launch_victim_scan(a, t, d_stop, d_panic, sc.stream));
  PROBE_TRY(kbg::launch_victim_big(a, t, d_rows, (int32_t)big_rows.size(), d_stop, d_panic, d_row_out, sc.stream));
  PROBE_TRY(hipStreamSynchronize(sc.stream));
  if (p->out_mode == 0) {
    memcpy(stop, h_stop, word_bytes);
    memcpy(panic, h_panic, word_bytes);
    memcpy(row_out, h_rows, row_bytes);
  } else {
    PROBE_TRY(hipMemcpy(stop, d_stop, word_bytes, hipMemcpyDeviceToHost));
    PROBE_TRY(hipMemcpy(panic, d_panic, word_bytes, hipMemcpyDeviceToHost));
  }
  PROBE_TRY(hipMemcpy(nodes, d, L * 56, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(c_run, t.c_run, P, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(j_ready, t.j_ready, J * 4, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(j_alloc, t.j_alloc, 3 * J * 8, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(q_alloc, t.q_alloc, 3 * Q * 8, hipMemcpyDeviceToHost));
  return 0;
}

// kbg_victim_why_kernel, then kbg_victim_why_big_kernel over the rows of
// [node_lo, node_lo + node_n) holding 129..kMaxNodeCandidates candidates, as
// kbg_victim_reasons runs them for nq queries at once.
struct kbg_probe_victim_why {
  int32_t n_nodes, W, node_lo, node_n;
  int32_t stride;   // rows of the node table block (row = node - node_lo)
  int32_t classes;  // rows of the per-class stage planes
  int32_t n_cand, n_jobs, n_queues;
  int32_t nq;       // queries
  int32_t n_rows;   // the caller's count of big rows; checked against the probe's own
};

// The flat tables of kbg_tool_probe_victim (no prep; class_mask is not read by
// these kernels), the stage planes (sel_ok, taint_ok [classes][W], unsched,
// live [W]) and nq queries (kbg::VictimScan records; n_nodes, W, node_lo and
// node_n of each must be the probe's). out: nq * kVictimWhyOut words + guard,
// device memory filled with the sentinel before the launch. The tables the
// kernels hold through non-const pointers (the node block, c_run, j_ready,
// j_alloc, q_alloc) are copied back so the caller sees them untouched.
extern "C" int32_t kbg_tool_probe_victim_why(const kbg_probe_victim_why* p, void* nodes, const uint8_t* panic_node,
                                             const uint64_t* planes, const int32_t* nt_off, const int32_t* c_jq,
                                             const double* c_req, uint8_t* c_run, const int32_t* j_min,
                                             int32_t* j_ready, double* j_alloc, double* q_alloc,
                                             const double* q_deserved, const double* drf_total,
                                             const kbg::VictimScan* queries, void* out) {
  t_error.clear();
  if (!p || !nodes || !panic_node || !planes || !nt_off || !c_jq || !c_req || !c_run || !j_min || !j_ready ||
      !j_alloc || !q_alloc || !q_deserved || !drf_total || !queries || !out)
    return reject("null argument");
  if (p->n_nodes < 1 || p->W < 1 || p->n_nodes > p->W * 64) return reject("n_nodes outside W");
  if (p->node_lo < 0 || (p->node_lo & 63)) return reject("node_lo not a multiple of 64");
  if (p->node_n < 1 || (int64_t)p->node_lo + p->node_n > p->n_nodes) return reject("node range outside n_nodes");
  if (p->stride < 1 || p->node_n > p->stride) return reject("node range outside the table block");
  if (p->classes < 1) return reject("no class");
  if (p->n_cand < 0 || p->n_jobs < 1 || p->n_queues < 1) return reject("empty tables");
  if (p->nq < 1 || p->nq > 65535) return reject("nq outside 1..65535");
  if (nt_off[0] != 0 || nt_off[p->n_nodes] != p->n_cand) return reject("nt_off does not span the candidates");
  for (int32_t n = 0; n < p->n_nodes; ++n)
    if (nt_off[n + 1] < nt_off[n]) return reject("nt_off not increasing");
  for (int32_t k = 0; k < p->n_cand; ++k)
    if (c_jq[2 * k] < 0 || c_jq[2 * k] >= p->n_jobs || c_jq[2 * k + 1] < 0 || c_jq[2 * k + 1] >= p->n_queues)
      return reject("candidate job or queue outside its table");
  for (int32_t i = 0; i < p->nq; ++i) {
    const kbg::VictimScan& q = queries[i];
    if (q.n_nodes != p->n_nodes || q.W != p->W || q.node_lo != p->node_lo || q.node_n != p->node_n)
      return reject("query: geometry differs from the probe's");
    if (q.cls < 0 || q.cls >= p->classes) return reject("query: cls outside the planes");
    if (q.mode < kbg::VM_PREEMPT_JOBS || q.mode > kbg::VM_RECLAIM) return reject("query: mode outside 0..2");
    if (q.n_tiers < 0 || q.n_tiers > kbg::kMaxVictimTiers) return reject("query: n_tiers outside 0..kMaxVictimTiers");
    for (int32_t k = 0; k < q.n_tiers; ++k)
      if (q.tier_fns[k] == 0 || (q.tier_fns[k] & ~(kbg::VP_GANG | kbg::VP_DRF | kbg::VP_PROP)))
        return reject("query: tier_fns outside the victim fns");
    if (q.job < 0 || q.job >= p->n_jobs || q.queue < 0 || q.queue >= p->n_queues)
      return reject("query: job or queue outside its table");
  }
  std::vector<int32_t> big_rows;
  for (int32_t n = p->node_lo; n < p->node_lo + p->node_n; ++n) {
    const int32_t L = nt_off[n + 1] - nt_off[n];
    if (L > 128 && L <= kbg::kMaxNodeCandidates) big_rows.push_back(n - p->node_lo);
  }
  if (p->n_rows != (int32_t)big_rows.size()) return reject("n_rows is not the number of big rows");

  Scope sc;
  PROBE_TRY(hipStreamCreate(&sc.stream));
  const size_t L = (size_t)p->stride, P = (size_t)p->n_cand, J = (size_t)p->n_jobs, Q = (size_t)p->n_queues;
  double* d = nullptr;
  PROBE_TRY(dev_copy(sc, (char**)&d, (const char*)nodes, L * 56));
  kbg::VictimTables t{};
  t.ntasks = (int32_t*)(d + 6 * L);
  t.maxtasks = (int32_t*)(d + 6 * L) + L;
  PROBE_TRY(dev_copy(sc, (uint8_t**)&t.panic_node, panic_node, (size_t)p->n_nodes));
  PROBE_TRY(dev_copy(sc, (uint64_t**)&t.class_mask, (const uint64_t*)nullptr, 2));  // not read by these kernels
  PROBE_TRY(dev_copy(sc, (int32_t**)&t.nt_off, nt_off, (size_t)p->n_nodes + 1));
  PROBE_TRY(dev_copy(sc, (int32_t**)&t.c_jq, c_jq, 2 * P));
  PROBE_TRY(dev_copy(sc, (double**)&t.c_req, c_req, 3 * P));
  PROBE_TRY(dev_copy(sc, &t.c_run, (const uint8_t*)c_run, P));
  PROBE_TRY(dev_copy(sc, (int32_t**)&t.j_queue, (const int32_t*)nullptr, J));  // not read by the kernels
  PROBE_TRY(dev_copy(sc, (int32_t**)&t.j_min, j_min, J));
  PROBE_TRY(dev_copy(sc, &t.j_ready, (const int32_t*)j_ready, J));
  PROBE_TRY(dev_copy(sc, &t.j_alloc, (const double*)j_alloc, 3 * J));
  PROBE_TRY(dev_copy(sc, &t.q_alloc, (const double*)q_alloc, 3 * Q));
  PROBE_TRY(dev_copy(sc, (double**)&t.q_deserved, q_deserved, 3 * Q));
  std::copy(drf_total, drf_total + 3, t.drf_total);
  int32_t* d_rows = nullptr;
  PROBE_TRY(dev_copy(sc, &d_rows, big_rows.data(), big_rows.size()));
  uint64_t* d_planes = nullptr;
  PROBE_TRY(dev_copy(sc, &d_planes, planes, kbg::kbg_stage_words(p->classes, p->W)));
  const kbg::StagePlanes sp = kbg::kbg_stage_planes(d_planes, p->classes, p->W);

  kbg::VictimWhyArgs a{};
  PROBE_TRY(dev_copy(sc, (kbg::VictimScan**)&a.q, queries, (size_t)p->nq));
  a.nq = p->nq;
  a.n_nodes = p->n_nodes;
  a.W = p->W;
  a.node_lo = p->node_lo;
  a.node_n = p->node_n;
  a.sel_ok = sp.sel_ok;
  a.taint_ok = sp.taint_ok;
  a.unsched = sp.unsched;
  a.live = sp.live;
  const size_t out_bytes = (size_t)p->nq * kbg::kVictimWhyOut * 4 + kProbeGuardBytes;
  PROBE_TRY(dev_copy(sc, (char**)&a.out, (const char*)nullptr, out_bytes, kProbeSentinel));

  PROBE_TRY(kbg::launch_victim_why(a, t, sc.stream));
  PROBE_TRY(kbg::launch_victim_why_big(a, t, d_rows, (int32_t)big_rows.size(), sc.stream));
  PROBE_TRY(hipStreamSynchronize(sc.stream));
  PROBE_TRY(hipMemcpy(out, a.out, out_bytes, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(nodes, d, L * 56, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(c_run, t.c_run, P, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(j_ready, t.j_ready, J * 4, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(j_alloc, t.j_alloc, 3 * J * 8, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(q_alloc, t.q_alloc, 3 * Q * 8, hipMemcpyDeviceToHost));
  return 0;
}

// kbg_task_why_init_kernel, then kbg_task_why_kernel, as kbg_task_reasons runs
// them for n_shapes shapes at once.
struct kbg_probe_task_why {
  int32_t n_nodes, W, tab_lo, tab_n;  // the table holds the global nodes [tab_lo, tab_lo + tab_n)
  int32_t stride;                     // rows of the node table block (row = node - tab_lo)
  int32_t classes;                    // rows of the per-class stage planes
  int32_t n_shapes, cap_check;
};

// The node table block (FirstFitArgs.nodes: 56 B per row of `stride`), the
// stage planes (sel_ok, taint_ok [classes][W], unsched, live [W]) and n_shapes
// kbg::TaskShape records. out: n_shapes * kTaskWhyOut words + guard, device
// memory filled with the sentinel before the launches. The node block is
// copied back so the caller sees it untouched.
extern "C" int32_t kbg_tool_probe_task_why(const kbg_probe_task_why* p, void* nodes, const uint64_t* planes,
                                           const kbg::TaskShape* shapes, void* out) {
  t_error.clear();
  if (!p || !nodes || !planes || !shapes || !out) return reject("null argument");
  if (p->n_nodes < 1 || p->W < 1 || p->n_nodes > p->W * 64) return reject("n_nodes outside W");
  if (p->tab_lo < 0 || (p->tab_lo & 63)) return reject("tab_lo not a multiple of 64");
  if (p->tab_n < 1 || (int64_t)p->tab_lo + p->tab_n > p->n_nodes) return reject("node range outside n_nodes");
  if (p->stride < 1 || p->tab_n > p->stride) return reject("node range outside the table block");
  if (p->classes < 1) return reject("no class");
  if (p->n_shapes < 1 || p->n_shapes > (1 << 20)) return reject("n_shapes outside 1..2^20");
  for (int32_t i = 0; i < p->n_shapes; ++i)
    if (shapes[i].cls < 0 || shapes[i].cls >= p->classes) return reject("shape: cls outside the planes");

  Scope sc;
  PROBE_TRY(hipStreamCreate(&sc.stream));
  const size_t L = (size_t)p->stride;
  double* d = nullptr;
  PROBE_TRY(dev_copy(sc, (char**)&d, (const char*)nodes, L * 56));
  uint64_t* d_planes = nullptr;
  PROBE_TRY(dev_copy(sc, &d_planes, planes, kbg::kbg_stage_words(p->classes, p->W)));
  const kbg::StagePlanes sp = kbg::kbg_stage_planes(d_planes, p->classes, p->W);
  kbg::TaskWhyArgs a{};
  a.nodes = d;
  a.stride = p->stride;
  a.W = p->W;
  a.tab_lo = p->tab_lo;
  a.tab_n = p->tab_n;
  a.sel_ok = sp.sel_ok;
  a.taint_ok = sp.taint_ok;
  a.unsched = sp.unsched;
  a.live = sp.live;
  PROBE_TRY(dev_copy(sc, (kbg::TaskShape**)&a.shapes, shapes, (size_t)p->n_shapes));
  a.n_shapes = p->n_shapes;
  a.cap_check = p->cap_check ? 1 : 0;
  const size_t out_bytes = (size_t)p->n_shapes * kbg::kTaskWhyOut * 4 + kProbeGuardBytes;
  PROBE_TRY(dev_copy(sc, (char**)&a.out, (const char*)nullptr, out_bytes, kProbeSentinel));

  PROBE_TRY(kbg::launch_task_why_init(a.out, a.n_shapes, sc.stream));
  PROBE_TRY(kbg::launch_task_why(a, sc.stream));
  PROBE_TRY(hipStreamSynchronize(sc.stream));
  PROBE_TRY(hipMemcpy(out, a.out, out_bytes, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(nodes, d, L * 56, hipMemcpyDeviceToHost));
  return 0;
}

// kbg_task_headroom_init_kernel, then kbg_task_headroom_kernel, as
// kbg_task_headroom runs them for n_shapes shapes at once.
struct kbg_probe_task_headroom {
  int32_t n_nodes, W, tab_lo, tab_n;  // the table holds the global nodes [tab_lo, tab_lo + tab_n)
  int32_t stride;                     // rows of the node table block (row = node - tab_lo)
  int32_t classes;                    // rows of the per-class stage planes
  int32_t n_shapes, cap_check;
  int32_t limit;  // copies counted per node at most, 1..kRoomMaxLimit
};

// The arrays of kbg_tool_probe_task_why. out: n_shapes * kRoomOut words +
// guard, device memory filled with the sentinel before the launches. A limit
// outside [1, kRoomMaxLimit] and tab_n * limit > INT32_MAX are refused here as
// launch_task_headroom refuses them. The node block is copied back so the
// caller sees it untouched.
extern "C" int32_t kbg_tool_probe_task_headroom(const kbg_probe_task_headroom* p, void* nodes, const uint64_t* planes,
                                                const kbg::TaskShape* shapes, void* out) {
  t_error.clear();
  if (!p || !nodes || !shapes || !out) return reject("null argument");
  if (!planes) return reject("null planes");
  if (p->n_nodes < 1 || p->W < 1 || p->n_nodes > p->W * 64) return reject("n_nodes outside W");
  if (p->tab_lo < 0 || (p->tab_lo & 63)) return reject("tab_lo not a multiple of 64");
  if (p->tab_n < 1 || (int64_t)p->tab_lo + p->tab_n > p->n_nodes) return reject("node range outside n_nodes");
  if (p->stride < 1 || p->tab_n > p->stride) return reject("node range outside the table block");
  if (p->classes < 1) return reject("no class");
  if (p->n_shapes < 1 || p->n_shapes > (1 << 20)) return reject("n_shapes outside 1..2^20");
  if (p->limit < 1 || p->limit > kbg::kRoomMaxLimit) return reject("limit outside 1..1024");
  if ((int64_t)p->tab_n * p->limit > INT32_MAX) return reject("tab_n * limit overflows a row's sums");
  for (int32_t i = 0; i < p->n_shapes; ++i)
    if (shapes[i].cls < 0 || shapes[i].cls >= p->classes) return reject("shape: cls outside the planes");

  Scope sc;
  PROBE_TRY(hipStreamCreate(&sc.stream));
  const size_t L = (size_t)p->stride;
  double* d = nullptr;
  PROBE_TRY(dev_copy(sc, (char**)&d, (const char*)nodes, L * 56));
  uint64_t* d_planes = nullptr;
  PROBE_TRY(dev_copy(sc, &d_planes, planes, kbg::kbg_stage_words(p->classes, p->W)));
  const kbg::StagePlanes sp = kbg::kbg_stage_planes(d_planes, p->classes, p->W);
  kbg::TaskRoomArgs a{};
  a.nodes = d;
  a.stride = p->stride;
  a.W = p->W;
  a.tab_lo = p->tab_lo;
  a.tab_n = p->tab_n;
  a.sel_ok = sp.sel_ok;
  a.taint_ok = sp.taint_ok;
  a.unsched = sp.unsched;
  a.live = sp.live;
  PROBE_TRY(dev_copy(sc, (kbg::TaskShape**)&a.shapes, shapes, (size_t)p->n_shapes));
  a.n_shapes = p->n_shapes;
  a.cap_check = p->cap_check ? 1 : 0;
  a.limit = p->limit;
  const size_t out_bytes = (size_t)p->n_shapes * kbg::kRoomOut * 4 + kProbeGuardBytes;
  PROBE_TRY(dev_copy(sc, (char**)&a.out, (const char*)nullptr, out_bytes, kProbeSentinel));

  PROBE_TRY(kbg::launch_task_headroom_init(a.out, a.n_shapes, sc.stream));
  PROBE_TRY(kbg::launch_task_headroom(a, sc.stream));
  PROBE_TRY(hipStreamSynchronize(sc.stream));
  PROBE_TRY(hipMemcpy(out, a.out, out_bytes, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(nodes, d, L * 56, hipMemcpyDeviceToHost));
  return 0;
}

// kbg_job_fit_kernel, as kbg_job_fit runs it for n_jobs walks at once.
thread_local double t_job_fit_ms = 0;  // the HIP-event time of the last launch (tools/job_fit_bench.py)
extern "C" double kbg_tool_probe_job_fit_ms() { return t_job_fit_ms; }

struct kbg_probe_job_fit {
  int32_t n_nodes, W, tab_lo, tab_n;  // the table holds the global nodes [tab_lo, tab_lo + tab_n)
  int32_t stride;                     // rows of the node table block (row = node - tab_lo)
  int32_t classes;                    // rows of the per-class stage planes
  int32_t n_shapes, cap_check;
  int32_t n_jobs, n_steps;  // job_off holds n_jobs + 1 offsets, the last n_steps
};

// The arrays of kbg_tool_probe_task_headroom, then the steps and the job
// offsets. out: n_steps * 2 words + guard, device memory filled with the
// sentinel before the launch. What launch_job_fit refuses is refused here by
// name (a table range past the bitmap before any array is read). The node
// block is copied back so the caller sees it untouched.
extern "C" int32_t kbg_tool_probe_job_fit(const kbg_probe_job_fit* p, void* nodes, const uint64_t* planes,
                                          const kbg::TaskShape* shapes, const kbg::JobFitStep* steps,
                                          const int32_t* job_off, void* out) {
  t_error.clear();
  if (!p || !nodes || !shapes || !steps || !job_off || !out) return reject("null argument");
  if (!planes) return reject("null planes");
  if (p->n_nodes < 1 || p->W < 1 || p->n_nodes > p->W * 64) return reject("n_nodes outside W");
  if (p->tab_lo < 0 || (p->tab_lo & 63)) return reject("tab_lo not a multiple of 64");
  if (p->tab_n < 1 || (int64_t)p->tab_lo + p->tab_n > p->n_nodes) return reject("node range outside n_nodes");
  if (p->stride < 1 || p->tab_n > p->stride) return reject("node range outside the table block");
  if (p->tab_n > kbg::kFitMaxNodes) return reject("table range past the touched-word bitmap");
  if (p->classes < 1) return reject("no class");
  if (p->n_shapes < 1 || p->n_shapes > (1 << 20)) return reject("n_shapes outside 1..2^20");
  if (p->n_jobs < 1 || p->n_jobs > (1 << 20)) return reject("n_jobs outside 1..2^20");
  if (p->n_steps < 0 || job_off[0] != 0 || job_off[p->n_jobs] != p->n_steps) return reject("job_off does not span n_steps");
  for (int32_t j = 0; j < p->n_jobs; ++j)
    if (job_off[j] > job_off[j + 1] || job_off[j + 1] > p->n_steps) return reject("job_off descends");
  for (int32_t i = 0; i < p->n_shapes; ++i)
    if (shapes[i].cls < 0 || shapes[i].cls >= p->classes) return reject("shape: cls outside the planes");

  kbg::JobFitArgs a{};
  a.stride = p->stride;
  a.W = p->W;
  a.tab_lo = p->tab_lo;
  a.tab_n = p->tab_n;
  a.n_shapes = p->n_shapes;
  a.n_jobs = p->n_jobs;
  a.cap_check = p->cap_check ? 1 : 0;
  a.h_shapes = shapes;
  a.h_steps = steps;
  a.h_job_off = job_off;
  if (const char* why = kbg::job_fit_refusal(a)) return reject(why);

  Scope sc;
  PROBE_TRY(hipStreamCreate(&sc.stream));
  const size_t L = (size_t)p->stride;
  double* d = nullptr;
  PROBE_TRY(dev_copy(sc, (char**)&d, (const char*)nodes, L * 56));
  uint64_t* d_planes = nullptr;
  PROBE_TRY(dev_copy(sc, &d_planes, planes, kbg::kbg_stage_words(p->classes, p->W)));
  const kbg::StagePlanes sp = kbg::kbg_stage_planes(d_planes, p->classes, p->W);
  a.nodes = d;
  a.sel_ok = sp.sel_ok;
  a.taint_ok = sp.taint_ok;
  a.unsched = sp.unsched;
  a.live = sp.live;
  PROBE_TRY(dev_copy(sc, (kbg::TaskShape**)&a.shapes, shapes, (size_t)p->n_shapes));
  PROBE_TRY(dev_copy(sc, (kbg::JobFitStep**)&a.steps, steps, (size_t)p->n_steps));
  PROBE_TRY(dev_copy(sc, (int32_t**)&a.job_off, job_off, (size_t)p->n_jobs + 1));
  const size_t out_bytes = (size_t)p->n_steps * 8 + kProbeGuardBytes;
  PROBE_TRY(dev_copy(sc, (char**)&a.out, (const char*)nullptr, out_bytes, kProbeSentinel));

  hipEvent_t ev[2] = {nullptr, nullptr};
  PROBE_TRY(hipEventCreate(&ev[0]));
  if (const hipError_t e = hipEventCreate(&ev[1]); e != hipSuccess) {
    (void)hipEventDestroy(ev[0]);
    return hip_fail(e, "hipEventCreate");
  }
  hipError_t e = kbg::launch_job_fit(a, sc.stream, ev[0], ev[1]);
  if (e == hipSuccess) e = hipStreamSynchronize(sc.stream);
  float ms = 0;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
  (void)hipEventDestroy(ev[0]);
  (void)hipEventDestroy(ev[1]);
  PROBE_TRY(e);
  t_job_fit_ms = ms;
  PROBE_TRY(hipMemcpy(out, a.out, out_bytes, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(nodes, d, L * 56, hipMemcpyDeviceToHost));
  return 0;
}

// kbg_node_why_init_kernel, then kbg_node_why_kernel, as kbg_node_reasons runs
// them for n_shapes shape records over the listed words at once.
thread_local double t_node_why_ms = 0;  // the HIP-event time of the last kbg_node_why_kernel launch
extern "C" double kbg_tool_probe_node_why_ms() { return t_node_why_ms; }

struct kbg_probe_node_why {
  int32_t n_nodes, W, tab_lo, tab_n;  // the table holds the global nodes [tab_lo, tab_lo + tab_n)
  int32_t stride;                     // rows of the node table block (row = node - tab_lo)
  int32_t classes;                    // rows of the per-class stage planes
  int32_t n_shapes, cap_check;
  int32_t n_words;  // entries of the word list
  int32_t ostride;  // words of an output plane, >= 64 * n_words
};

// The arrays of kbg_tool_probe_task_why with kbg::NodeWhyShape records, and
// the word list (words of the table, ascending, no repeats). out:
// kNodeWhyFields * ostride words + guard, device memory filled with the
// sentinel before the launches. Refused (-2) is what kbg_node_reasons never
// launches: a weight < 1, weight_open outside [0, weight], a negative
// first_task, weights summing past INT32_MAX, a word list that is unsorted,
// repeats a word or leaves the table, planes too short for the list. The node
// block is copied back so the caller sees it untouched.
extern "C" int32_t kbg_tool_probe_node_why(const kbg_probe_node_why* p, void* nodes, const uint64_t* planes,
                                           const kbg::NodeWhyShape* shapes, const int32_t* words, void* out) {
  t_error.clear();
  if (!p || !nodes || !planes || !shapes || !words || !out) return reject("null argument");
  if (p->n_nodes < 1 || p->W < 1 || p->n_nodes > p->W * 64) return reject("n_nodes outside W");
  if (p->tab_lo < 0 || (p->tab_lo & 63)) return reject("tab_lo not a multiple of 64");
  if (p->tab_n < 1 || (int64_t)p->tab_lo + p->tab_n > p->n_nodes) return reject("node range outside n_nodes");
  if (p->stride < 1 || p->tab_n > p->stride) return reject("node range outside the table block");
  if (p->classes < 1) return reject("no class");
  if (p->n_shapes < 1 || p->n_shapes > (1 << 20)) return reject("n_shapes outside 1..2^20");
  int64_t sum = 0;
  for (int32_t i = 0; i < p->n_shapes; ++i) {
    const kbg::NodeWhyShape& r = shapes[i];
    if (r.sh.cls < 0 || r.sh.cls >= p->classes) return reject("shape: cls outside the planes");
    if (r.weight < 1) return reject("shape: weight below 1");
    if (r.weight_open < 0 || r.weight_open > r.weight) return reject("shape: weight_open outside 0..weight");
    if (r.first_task < 0) return reject("shape: negative first_task");
    if ((sum += r.weight) > INT32_MAX) return reject("the weights sum past INT32_MAX");
  }
  const int32_t tab_words = (p->tab_n + 63) >> 6;
  if (p->n_words < 1 || p->n_words > tab_words) return reject("word list: n_words outside 1..the table's words");
  for (int32_t i = 0; i < p->n_words; ++i) {
    if (words[i] < 0 || words[i] >= tab_words) return reject("word list: a word outside the table");
    if (i && words[i] <= words[i - 1]) return reject("word list: not ascending or a word twice");
  }
  if (p->ostride < p->n_words * 64) return reject("ostride below 64 * n_words");
  if ((int64_t)p->ostride * kbg::kNodeWhyFields * 4 > (1ll << 30)) return reject("ostride too large");

  Scope sc;
  PROBE_TRY(hipStreamCreate(&sc.stream));
  const size_t L = (size_t)p->stride;
  double* d = nullptr;
  PROBE_TRY(dev_copy(sc, (char**)&d, (const char*)nodes, L * 56));
  uint64_t* d_planes = nullptr;
  PROBE_TRY(dev_copy(sc, &d_planes, planes, kbg::kbg_stage_words(p->classes, p->W)));
  const kbg::StagePlanes sp = kbg::kbg_stage_planes(d_planes, p->classes, p->W);
  kbg::NodeWhyArgs a{};
  a.nodes = d;
  a.stride = p->stride;
  a.W = p->W;
  a.tab_lo = p->tab_lo;
  a.tab_n = p->tab_n;
  a.sel_ok = sp.sel_ok;
  a.taint_ok = sp.taint_ok;
  a.unsched = sp.unsched;
  a.live = sp.live;
  PROBE_TRY(dev_copy(sc, (kbg::NodeWhyShape**)&a.shapes, shapes, (size_t)p->n_shapes));
  a.n_shapes = p->n_shapes;
  a.cap_check = p->cap_check ? 1 : 0;
  PROBE_TRY(dev_copy(sc, (int32_t**)&a.words, words, (size_t)p->n_words));
  a.n_words = p->n_words;
  a.ostride = p->ostride;
  const size_t out_bytes = (size_t)p->ostride * kbg::kNodeWhyFields * 4 + kProbeGuardBytes;
  PROBE_TRY(dev_copy(sc, (char**)&a.out, (const char*)nullptr, out_bytes, kProbeSentinel));

  hipEvent_t ev[2] = {nullptr, nullptr};
  PROBE_TRY(hipEventCreate(&ev[0]));
  if (const hipError_t e = hipEventCreate(&ev[1]); e != hipSuccess) {
    (void)hipEventDestroy(ev[0]);
    return hip_fail(e, "hipEventCreate");
  }
  hipError_t e = kbg::launch_node_why_init(a.out, a.ostride, a.n_words, sc.stream);
  if (e == hipSuccess) e = kbg::launch_node_why(a, sc.stream, ev[0], ev[1]);
  if (e == hipSuccess) e = hipStreamSynchronize(sc.stream);
  float ms = 0;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
  (void)hipEventDestroy(ev[0]);
  (void)hipEventDestroy(ev[1]);
  PROBE_TRY(e);
  t_node_why_ms = ms;
  PROBE_TRY(hipMemcpy(out, a.out, out_bytes, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(nodes, d, L * 56, hipMemcpyDeviceToHost));
  return 0;
}

// kbg_drain_kernel, as kbg_node_drain runs it for n_walks walks at once.
thread_local double t_drain_ms = 0;  // the HIP-event time of the last launch (tools/drain_bench.py)
extern "C" double kbg_tool_probe_drain_ms() { return t_drain_ms; }

struct kbg_probe_drain {
  int32_t n_nodes, W, tab_lo, tab_n;  // the table holds the global nodes [tab_lo, tab_lo + tab_n)
  int32_t stride;                     // rows of the node table block (row = node - tab_lo)
  int32_t classes;                    // rows of the per-class stage planes
  int32_t n_shapes, cap_check;
  int32_t n_walks, n_steps;  // walk_off holds n_walks + 1 offsets, the last n_steps
};

// The arrays of kbg_tool_probe_job_fit, then the excluded plane (W words over
// the global nodes) and each walk's excluded table row. out: n_steps * 2 words
// + guard, device memory filled with the sentinel before the launch. What
// launch_drain refuses is refused here by name (a table range past the bitmap
// before any array is read). The node block and the planes are copied back so
// the caller sees them untouched.
extern "C" int32_t kbg_tool_probe_drain(const kbg_probe_drain* p, void* nodes, uint64_t* planes,
                                        const kbg::TaskShape* shapes, const kbg::JobFitStep* steps,
                                        const int32_t* walk_off, const uint64_t* excl, const int32_t* walk_row,
                                        void* out) {
  t_error.clear();
  if (!p || !nodes || !shapes || !steps || !walk_off || !excl || !walk_row || !out) return reject("null argument");
  if (!planes) return reject("null planes");
  if (p->n_nodes < 1 || p->W < 1 || p->n_nodes > p->W * 64) return reject("n_nodes outside W");
  if (p->tab_lo < 0 || (p->tab_lo & 63)) return reject("tab_lo not a multiple of 64");
  if (p->tab_n < 1 || (int64_t)p->tab_lo + p->tab_n > p->n_nodes) return reject("node range outside n_nodes");
  if (p->stride < 1 || p->tab_n > p->stride) return reject("node range outside the table block");
  if (p->tab_n > kbg::kFitMaxNodes) return reject("table range past the touched-word bitmap");
  if (p->classes < 1) return reject("no class");
  if (p->n_shapes < 1 || p->n_shapes > (1 << 20)) return reject("n_shapes outside 1..2^20");
  if (p->n_walks < 1 || p->n_walks > kbg::kDrainMaxWalks) return reject("n_walks outside 1..2^20");
  if (p->n_steps < 0 || walk_off[0] != 0 || walk_off[p->n_walks] != p->n_steps)
    return reject("walk_off does not span n_steps");
  for (int32_t j = 0; j < p->n_walks; ++j)
    if (walk_off[j] > walk_off[j + 1] || walk_off[j + 1] > p->n_steps) return reject("walk_off descends");
  for (int32_t i = 0; i < p->n_shapes; ++i)
    if (shapes[i].cls < 0 || shapes[i].cls >= p->classes) return reject("shape: cls outside the planes");

  kbg::DrainArgs a{};
  a.stride = p->stride;
  a.W = p->W;
  a.tab_lo = p->tab_lo;
  a.tab_n = p->tab_n;
  a.n_shapes = p->n_shapes;
  a.n_walks = p->n_walks;
  a.cap_check = p->cap_check ? 1 : 0;
  a.h_shapes = shapes;
  a.h_steps = steps;
  a.h_walk_off = walk_off;
  a.h_walk_row = walk_row;
  if (const char* why = kbg::drain_refusal(a)) return reject(why);

  Scope sc;
  PROBE_TRY(hipStreamCreate(&sc.stream));
  const size_t L = (size_t)p->stride;
  double* d = nullptr;
  PROBE_TRY(dev_copy(sc, (char**)&d, (const char*)nodes, L * 56));
  uint64_t* d_planes = nullptr;
  const size_t plane_words = kbg::kbg_stage_words(p->classes, p->W);
  PROBE_TRY(dev_copy(sc, &d_planes, (const uint64_t*)planes, plane_words));
  const kbg::StagePlanes sp = kbg::kbg_stage_planes(d_planes, p->classes, p->W);
  a.nodes = d;
  a.sel_ok = sp.sel_ok;
  a.taint_ok = sp.taint_ok;
  a.unsched = sp.unsched;
  a.live = sp.live;
  PROBE_TRY(dev_copy(sc, (uint64_t**)&a.excl, excl, (size_t)p->W));
  PROBE_TRY(dev_copy(sc, (kbg::TaskShape**)&a.shapes, shapes, (size_t)p->n_shapes));
  PROBE_TRY(dev_copy(sc, (kbg::JobFitStep**)&a.steps, steps, (size_t)p->n_steps));
  PROBE_TRY(dev_copy(sc, (int32_t**)&a.walk_off, walk_off, (size_t)p->n_walks + 1));
  PROBE_TRY(dev_copy(sc, (int32_t**)&a.walk_row, walk_row, (size_t)p->n_walks));
  const size_t out_bytes = (size_t)p->n_steps * 8 + kProbeGuardBytes;
  PROBE_TRY(dev_copy(sc, (char**)&a.out, (const char*)nullptr, out_bytes, kProbeSentinel));

  hipEvent_t ev[2] = {nullptr, nullptr};
  PROBE_TRY(hipEventCreate(&ev[0]));
  if (const hipError_t e = hipEventCreate(&ev[1]); e != hipSuccess) {
    (void)hipEventDestroy(ev[0]);
    return hip_fail(e, "hipEventCreate");
  }
  hipError_t e = kbg::launch_drain(a, sc.stream, ev[0], ev[1]);
  if (e == hipSuccess) e = hipStreamSynchronize(sc.stream);
  float ms = 0;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
  (void)hipEventDestroy(ev[0]);
  (void)hipEventDestroy(ev[1]);
  PROBE_TRY(e);
  t_drain_ms = ms;
  PROBE_TRY(hipMemcpy(out, a.out, out_bytes, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(nodes, d, L * 56, hipMemcpyDeviceToHost));
  PROBE_TRY(hipMemcpy(planes, d_planes, plane_words * 8, hipMemcpyDeviceToHost));
  return 0;
}
