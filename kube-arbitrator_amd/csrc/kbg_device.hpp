// Device-side data layout and kernel launchers of the MI355X allocate path.
//
// Node table (HBM, struct-of-arrays, one entry per ssn.Nodes position):
//   idle_{cpu,mem,gpu}, rel_{cpu,mem,gpu}  f64[N]   NodeInfo.Idle / .Releasing
//   ntasks, maxtasks                       i32[N]   len(NodeInfo.Tasks), Allocatable.MaxTaskNum
// 56 B of dynamic state per node; the static part of the predicate
// (selector/affinity, taints, unschedulable) is resolved once per session into
// class_mask[class][word] (1 bit per node) by kbg_build_class_mask.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kbg {

// resource_info.go:54-56 LessEqual tolerances
constexpr double kMinMilliCPU = 10.0;
constexpr double kMinMemory = 10.0 * 1024.0 * 1024.0;
constexpr double kMinMilliGPU = 10.0;

// select kernel result encoding
constexpr uint32_t kCandPipelineBit = 0x80000000u;  // candidate fits Releasing only
constexpr uint32_t kCountIncompleteBit = 0x40000000u;
constexpr uint32_t kCountMask = 0x3fffffffu;

struct NodeSoA {
  double* idle_cpu;
  double* idle_mem;
  double* idle_gpu;
  double* rel_cpu;
  double* rel_mem;
  double* rel_gpu;
  int32_t* ntasks;
  int32_t* maxtasks;
};

// One task evaluation request (32 B, SURVEY §8(d) task record).
// General mode: req = Resreq and the kernel evaluates LessEqual with the
// reference's expression `r < a || |a - r| < min` per dimension.
// Integer mode (the session proved every node value and request an exact
// integer of magnitude <= 2^51, with the pending requests' sum <= 2^51 so the
// values stay exact integers for the whole cycle): req = Resreq - min, and
// `r <= a` is exactly `a > req`: if r < a then a > r - min; if |a - r| < min
// then a - r > -min; conversely a > r - min gives r < a or r - min < a <= r,
// i.e. |a - r| < min — every operation exact on such integers.
struct TaskRec {
  double req[3];
  int32_t cls;
  int32_t flags;  // kRowRelZeroFits: LessEqual(Resreq, 0) (the Releasing fit on a zero-Releasing node)
};
constexpr int32_t kRowRelZeroFits = 1;

// Scan rows per workgroup (one per lane for the write-out). The host pads
// every batch's rows to a multiple of this with copies of a real row, so the
// kernel's row loop has no bound checks (kbg_pad_rows).
constexpr int kScanRowsPerBlock = 64;
inline int32_t kbg_pad_rows(int32_t g) { return (g + kScanRowsPerBlock - 1) / kScanRowsPerBlock * kScanRowsPerBlock; }

// Node row written back after the host commits placements (AddTask delta).
struct NodeDelta {
  int32_t node;
  int32_t ntasks;
  double idle[3];
  double rel[3];
  int32_t maxtasks;  // Allocatable pods (changes only through a session update)
  int32_t pad;
};

// One class-mask word rewritten by the host (host-port conflicts).
struct MaskDelta {
  uint32_t index;
  uint32_t pad;
  uint64_t value;
};
constexpr int32_t kMaskDeltaCap = 8192;

// ---- preempt / reclaim victim scan (preempt.go:182-240, reclaim.go:106-135)
enum VictimPlugin : int32_t { VP_GANG = 1, VP_DRF = 2, VP_PROP = 4 };
enum VictimMode : int32_t { VM_PREEMPT_JOBS = 0, VM_PREEMPT_TASKS = 1, VM_RECLAIM = 2 };
constexpr int kMaxVictimTiers = 8;
constexpr int kVictimChunks = 16;                      // 64-candidate chunks per node in one victim scan
constexpr int kMaxNodeCandidates = 64 * kVictimChunks;  // victim candidates per node

// One reclaimer / preemptor against every node.
struct VictimScan {
  int32_t n_nodes, W, cls, cap_check;  // n_nodes: global N
  int32_t node_lo, node_n;             // node range this launch covers (the shard's node table, tab_lo based)
  int32_t mode;                        // VictimMode
  int32_t n_tiers;                     // tiers holding an enabled victim fn, in order
  int32_t tier_fns[kMaxVictimTiers];   // VictimPlugin bits of each (every fn keeps the preemptee order,
                                       // so the intersection does not depend on the fns' order)
  int32_t job, queue;                  // the preemptor's
  double req[3];                       // its Resreq
  double ls;                           // drf: its job's share with it placed
};

struct VictimTables {
  const int32_t* ntasks;        // node table rows (node - VictimScan.node_lo)
  const int32_t* maxtasks;
  const uint8_t* panic_node;    // nil Node under an active predicates plugin
  const uint64_t* class_mask;
  const int32_t* nt_off;        // [N+1] candidate lists: session tasks Running on the node at open,
                                //       in NodeInfo.Tasks order; position p = nt_off[n] + k
  const int2* c_jq;             // [P] {job, queue} of the candidate at position p (coalesced per lane)
  const double* c_req;          // [P][3] its Resreq
  uint8_t* c_run;               // [P] node-side status still Running
  const int32_t* j_queue;       // per job
  const int32_t* j_min;
  int32_t* j_ready;             // gang readyTaskNum
  double* j_alloc;              // [J][3] drf attr.allocated
  double* q_alloc;              // [Q][3] proportion attr.allocated
  const double* q_deserved;     // [Q][3]
  double drf_total[3];
};

// A host-side change to the victim tables.
struct StateDelta {
  int32_t kind;   // 0 candidate running flag (index = candidate position), 1 job ready, 2 job drf alloc, 3 queue alloc
  int32_t index;
  double v[3];
};

// ---- static predicate programs (built on host, evaluated on device) ----
enum ReqKind : int32_t {
  REQ_FALSE = 0,
  REQ_TRUE = 1,
  REQ_ALL = 2,      // (label_bits & mask) == mask
  REQ_ANY = 3,      // (label_bits & mask) != 0
  REQ_NONE = 4,     // (label_bits & mask) == 0
  REQ_GT = 5,       // numeric label column > value
  REQ_LT = 6,       // numeric label column < value
  REQ_NAME_EQ = 7,  // node name id == value
  REQ_NAME_NE = 8,  // node name id != value
};

struct ReqProg {
  int32_t kind;
  int32_t mask_off;  // offset (in u64 words) into the mask pool, label_words wide
  int32_t col;       // numeric column for GT/LT
  int32_t pad;
  int64_t value;
};

struct TermProg {
  int32_t req_off, req_len;  // AND of reqs; a skipped term is not emitted
};

struct ClassProg {
  int32_t sel_req;           // index of the nodeSelector requirement, -1 = none
  int32_t has_affinity;      // required node affinity present: OR over terms
  int32_t term_off, term_len;
  int32_t tol_off;           // offset into the tolerated-mask pool (taint_words wide)
  int32_t always;            // 1 = predicate always true for this class (predicates inactive)
};

struct StaticTables {
  int32_t n_nodes;
  int32_t label_words;       // u64 words per node label bitset
  int32_t taint_words;       // u64 words per node taint bitset
  int32_t n_numcols;
  const uint64_t* label_bits;    // [label_words][N]  (word-major => coalesced)
  const uint64_t* taint_bits;    // [taint_words][N]
  const int64_t* num_vals;       // [n_numcols][N]
  const uint8_t* num_ok;         // [n_numcols][N]
  const int32_t* name_id;        // [N]
  const uint8_t* node_flags;     // [N] bit0 = unschedulable, bit1 = nil Node, bit2 = ghost-failed
  const uint64_t* mask_pool;
  const uint64_t* tol_pool;
  const ReqProg* reqs;
  const TermProg* terms;
  const ClassProg* classes;
};

enum NodeFlag : uint8_t { NF_UNSCHED = 1, NF_NIL = 2, NF_DEAD = 4 };

// ---- launchers (all asynchronous on `stream`) ----
hipError_t launch_build_class_mask(const StaticTables& t, int32_t n_classes, int32_t W, uint64_t* class_mask,
                                   hipStream_t stream);

// Words a row takes in one shard slot of the feasibility bitmaps: Wl rounded
// up to whole quads (a quad = the 4 words one scan workgroup produces).
__host__ __device__ inline int32_t kbg_slot_words(int32_t Wl) { return (Wl + 3) & ~3; }

// Feasibility bitmaps of a batch of G evaluation rows live in one buffer laid
// out [slot][plane][quad][row][4] (u64 words; plane 0 = Idle-or-Releasing
// fit, plane 1 = Idle fit; slot = node-axis shard of Wl 64-node words, quad
// = 4 consecutive words of it, kbg_slot_words(Wl) / 4 quads per row). A scan
// workgroup writes its rows' quad as one contiguous run, so no cache line is
// shared between workgroups (or XCDs). Unsharded, slot count 1 and Wl = W.
// Sharded, the per-shard slots are exactly an all-gather's receive layout, so
// the select kernel reads the same buffer whether the slots were written
// locally or gathered over RCCL.

struct ScanGeom {
  int32_t n_nodes;   // global node count N
  int32_t W;         // global 64-node words, ceil(N/64)
  int32_t Wl;        // words per shard slot
  int32_t chunk_lo;  // first global word this launch covers
  int32_t n_chunks;  // words this launch covers (Wl for one shard; slots*Wl for all local shards)
  int32_t tab_lo;    // first global node held by the node table (rows are node - tab_lo)
};

// `start`/`stop` (optional) are stamped at the kernel's own start and end
// (hipExtLaunchKernelGGL), so their elapsed time is the kernel duration.
// `out` points at the slot of chunk_lo.
hipError_t launch_scan(const NodeSoA& n, const ScanGeom& g, const uint64_t* class_mask, const TaskRec* tasks,
                       int32_t n_tasks, int32_t cap_check, int32_t int_mode, uint64_t* out, hipStream_t stream,
                       hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

// The fused scan + first-fit extraction (kbg_firstfit_kernel). Rows map to
// shapes: row g evaluates shape s = row_shape[g] & ~kRowWriter (grouped mode:
// row_shape null, s = g, every row a writer). A shape is a TaskRec whose
// flags carry kRowRelZeroFits and, from bit kRowWantShift, `want`: how many
// fits its list must hold before the walk may stop (EARLY_EXIT) and the
// output may end. The writer row of shape s writes, for the words [w_lo,
// w_lo + covered) in node order, the pair of 64-node masks {fits Idle or
// Releasing, fits Idle} (static predicate, pod cap and LessEqual applied)
// into masks[s * mw + (w - mask_w0)], and info[s * info_stride + part0 + part] = covered |
// kInfoAnyBit (some node of the part's walked words fits) |
// kCountIncompleteBit (covered < the part's words: the list is cut after the
// word holding its want-th fit; never with `complete`). Every fit of
// a covered word is in the masks, so the host reads the first-fit candidates
// in node order by scanning bits. The shape table is in the kernel arguments
// (n_shapes <= kInlineShapes: no PCIe read at launch) or host-mapped;
// row_shape, info, masks, avail may be host-mapped (zero-copy).
constexpr int kInlineShapes = 96;
constexpr int kFfRoundWords = 128;  // words per round of the fused walk (one round: no early exit)
constexpr int kFfMaxSplits = 8;
constexpr uint32_t kRowWriter = 0x80000000u;
constexpr int kRowWantShift = 1;
constexpr uint32_t kInfoAnyBit = 0x20000000u;
constexpr uint32_t kInfoWordsMask = 0x00ffffffu;
struct alignas(16) MaskPair {
  uint64_t f;  // fits Idle or Releasing
  uint64_t i;  // fits Idle
};
struct FirstFitArgs {
  const double* nodes;          // the node table as one block (NodeSoA of alloc_soa): rows of the nodes
                                // [tab_lo, tab_lo + tab_n), idle c/m/g, rel c/m/g f64[stride], ntasks,
                                // maxtasks i32[stride]
  const uint64_t* class_mask;   // [class][W]
  const TaskRec* shapes;        // host-mapped shape table, or null: inl[]
  const uint32_t* row_shape;    // [G] shape | kRowWriter, or null: row g is shape g and writes it
  uint32_t* info;               // [n_shapes]
  MaskPair* masks;              // [n_shapes][mw]
  uint32_t* avail;              // owner-resolve: [n_shapes] avail_bit when any node fits, else 0
  uint32_t avail_bit;
  int32_t stride, G, n_shapes, mw;
  int32_t n_nodes, W, w_lo, w_hi, tab_lo, tab_n;
  int32_t cap_check;            // the predicates plugin's pod cap is on
  int32_t early_exit;           // stop once every row's list is full (production mode)
  int32_t complete;             // every word's masks go out (want ignored): lists are never cut
  int32_t splits, split_words;  // the words [w_lo, w_hi) in `splits` parts of split_words, one workgroup
                                // each (a short batch's walk spread over more CUs); info is per (shape, part)
  int32_t rows;                 // rows per workgroup (firstfit_geometry; at most the kernel's ROWS)
  int32_t info_stride, part0;   // info[s * info_stride + part0 + part] (a single launch: splits, 0; a rank of
                                // the scan service: every rank's parts, this rank's first)
  int32_t mask_w0;              // the global word masks[s * mw] holds (w_lo; 0 under the scan service)
  int32_t runs;                 // full-scan with inline shapes: launch row l belongs to the slot s with
                                // run_end[s - 1] <= l < run_end[s] and the run's last row writes the slot
                                // (no row -> shape map to read: rows of a slot are identical evaluations)
  TaskRec inl[kInlineShapes];
  uint16_t run_end[kInlineShapes];
};
// Launch geometry of G rows: the kernel's rows-per-workgroup variant (16, 24
// or 32) and the rows each workgroup takes (<= that). Production (grouped)
// batches take whole 16/24/32-row blocks; full-scan batches spread their rows
// evenly over the 256 CUs (ceil(G / 256) rounded up to a pair), so a launch of
// 4.2k rows runs 17-18 rows on each CU instead of 24 on 174 of them.
struct FfGeometry {
  int32_t variant, rows;
};
FfGeometry firstfit_geometry(int32_t G, bool full_scan);
hipError_t launch_firstfit(const FirstFitArgs& a, int32_t int_mode, hipStream_t stream, hipEvent_t start = nullptr,
                           hipEvent_t stop = nullptr);


// Row g gets cap_off[g+1]-cap_off[g] candidate slots at out_cand[cap_off[g]],
// taken from the global words [w_lo, w_hi) in node order.
hipError_t launch_select(const uint64_t* bits, int32_t w_lo, int32_t w_hi, int32_t Wl, int32_t n_rows,
                         const uint32_t* cap_off, uint32_t* out_cand, uint32_t* out_count, hipStream_t stream,
                         hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

hipError_t launch_apply(const NodeSoA& n, const NodeDelta* deltas, int32_t n_deltas, hipStream_t stream);
// dst[0..n16) = src[0..n16), 16 B per lane (the node-table restore of kbg_session_reset)
hipError_t launch_copy16(void* dst, const void* src, size_t n16, hipStream_t stream);

// FitError counts of not-ready jobs (kbg_fitdelta_kernel).
struct FitQuery {
  int32_t cls, end, point, win;  // static class; nodes [0, end); decisions before `point` applied; the winner
  double req[3];                 // Resreq
};
struct FitArgs {
  const double* nodes;         // the final node table block (FirstFitArgs.nodes)
  int32_t stride, W;
  const uint64_t* class_mask;  // static predicate [class][W]
  const int32_t* hoff;         // [N + 1] each node's decisions
  const int32_t* hk;           // decision index | 0x80000000 for a Pipeline
  const double* hold;          // [3] per decision: the Idle (Allocate) / Releasing (Pipeline) before it
  const int32_t* na;           // per decision: the first Allocate at or after it on its node, -1 none
  const FitQuery* q;
  int32_t nq, cap_check;
  int32_t* out;                // [nq][4]: entries, negative cpu, memory, GPU deltas (host-mapped)
  int32_t tab_lo, tab_n;       // the global nodes the table holds (a shard of the scan service: its own)
};
hipError_t launch_fitdelta(const FitArgs& a, hipStream_t stream);

// Per-predicate unschedulable reasons (kbg_job_reasons). The static predicate
// split by stage, one bit per node (kbg_stage_mask_kernel): sel_ok and
// taint_ok per class, unsched and live per table, every stage evaluated on its
// own, so for a class that is not `always`
//   class_mask == sel_ok & taint_ok & ~unsched & live
// (a nil Node passes every stage, as in kbg_mask_kernel: the host reports it).
struct StagePlanes {
  uint64_t* sel_ok;    // [class][W] node selector + required node affinity hold
  uint64_t* taint_ok;  // [class][W] every NoSchedule / NoExecute taint is tolerated
  uint64_t* unsched;   // [W] Spec.Unschedulable
  uint64_t* live;      // [W] the node is in ssn.Nodes (not deleted)
};
inline size_t kbg_stage_words(int32_t n_classes, int32_t W) { return (2 * (size_t)n_classes + 2) * (size_t)W; }
inline StagePlanes kbg_stage_planes(uint64_t* block, int32_t n_classes, int32_t W) {
  const size_t cw = (size_t)n_classes * W;
  return StagePlanes{block, block + cw, block + 2 * cw, block + 2 * cw + W};
}
hipError_t launch_build_stage_planes(const StaticTables& t, int32_t n_classes, int32_t W, const StagePlanes& p,
                                     hipStream_t stream);
// kbg_reasons_kernel: per FitError query (FitArgs' staging: hoff, hk, q) the
// live nodes of the visited range [0, win + 1) (win < 0: [0, end)) counted by
// the first failing stage in the reference's order; the nodes at or after
// `end` (the node an Allocate took) are visited only. out[q][kReasonOut]:
// visited, count[6], first_node[6] (KBG_WHY_* order; host ports and pod
// affinity stay 0 / -1 here: such sessions take the host path).
constexpr int kReasonOut = 16;
struct ReasonArgs {
  const double* nodes;  // the final node table block (its pod counts and caps)
  int32_t stride, W;
  const uint64_t *sel_ok, *taint_ok, *unsched, *live;  // StagePlanes
  const int32_t* hoff;
  const int32_t* hk;
  const FitQuery* q;
  int32_t nq, cap_check;  // cap_check 0 (predicates off): every count 0
  int32_t* out;           // [nq][kReasonOut] (host-mapped)
  int32_t tab_lo, tab_n;
};
hipError_t launch_reasons(const ReasonArgs& a, hipStream_t stream, hipEvent_t start = nullptr,
                          hipEvent_t stop = nullptr);
hipError_t launch_mask_apply(uint64_t* class_mask, const MaskDelta* deltas, int32_t n_deltas, hipStream_t stream);

// One victim scan evaluates every node of the range for one (preemptor,
// state) and writes two bitmaps of 32-node words, indexed by global node:
// stop[n] — the reference would stop at node n (validated victims, or a
// panic), panic[n] — that stop is a panic. The reference's answer is the
// lowest stop; the host keeps the maps and, as later tries of the same
// preemptor shape change the state, re-evaluates only the nodes those changes
// touched (kbg_session.cpp VictimCache). A workgroup (16 waves) covers 32
// consecutive nodes, two per wave, and writes its two words; sharded, each
// rank writes the words of its node range (64-node aligned) into zeroed
// arrays and an element-wise ncclAllReduce(max) of disjoint words is their OR.
constexpr int kVictimNodesPerBlock = 8;  // one node per wave; a workgroup writes one byte of stop bits
constexpr int kVictimBlockWaves = 8;
inline int32_t kbg_victim_words(int32_t n_nodes) { return (n_nodes + 31) / 32; }
hipError_t launch_victim_scan(const VictimScan& p, const VictimTables& t, uint32_t* stop_bits, uint32_t* panic_bits,
                              hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// Nodes of the scanned range with more than 128 candidates (`rows`, table
// rows), evaluated after launch_victim_scan: ORed into its device words, or
// (row_out non-null) one byte per row, bit 0 stop and bit 1 panic.
hipError_t launch_victim_big(const VictimScan& p, const VictimTables& t, const int32_t* rows, int32_t n_rows,
                             uint32_t* stop_bits, uint32_t* panic_bits, uint8_t* row_out, hipStream_t stream);
// Host-side changes before a scan, read in place from host-mapped memory:
// node rows (NodeInfo.Tasks count / Idle / Releasing) and victim-table
// entries, in one launch.
hipError_t launch_victim_prep(const NodeSoA& n, const VictimTables& t, const NodeDelta* nd, int32_t n_nodes,
                              const StateDelta* sd, int32_t n_state, hipStream_t stream);
// The common case (a try evicted a few tasks) carried in the kernel arguments:
// no PCIe reads on the critical path.
constexpr int kArgNodeDeltas = 16;
constexpr int kArgStateDeltas = 48;
struct VictimPrepArgs {
  int32_t nn, ns;
  NodeDelta nd[kArgNodeDeltas];
  StateDelta sd[kArgStateDeltas];
};
hipError_t launch_victim_prep_inline(const NodeSoA& n, const VictimTables& t, const VictimPrepArgs& a,
                                     hipStream_t stream);

// Why a victim scan found nothing (kbg_victim_reasons). Every live node of
// the range goes under exactly one cause for each of nq queries (a query is a
// VictimScan; all of a launch share n_nodes, W, node_lo and node_n), the first
// that applies:
//   a node whose `live` bit is clear is not counted at all;
//   panic_node                                          -> kWhyPanic;
//   cap_check: ntasks >= maxtasks -> 0 (pod cap), sel_ok clear -> 1,
//     unsched set -> 3, taint_ok clear -> 4 (KBG_WHY_* codes; class_mask is
//     not read: the stage planes name the stage);
//   no Running candidate passes the mode's filter        -> kWhyNoPreemptees;
//   a Sub underflow in a tier the walk reaches           -> kWhyPanic;
//   every tier's intersection empty, or n_tiers == 0     -> kWhyNoVictims;
//   the victims' sum Less than req                       -> kWhyNotEnough;
//   otherwise                                            -> kWhyVictims.
// Row q of `out` (kVictimWhyOut words): count[kWhyCauses], first_node
// [kWhyCauses] (lowest global node of the cause, -1 none), fn_empty[3]: the
// kWhyNoVictims nodes on which fn f (gang, drf, proportion), enabled in some
// tier, keeps nobody of the node's whole preemptee list by itself.
// launch_victim_why sets every row to its empty value and counts the nodes of
// up to 128 candidates; launch_victim_why_big, after it on the same stream,
// adds the rows of 129..kMaxNodeCandidates candidates (launch_victim_big's
// list). Nodes holding more are in neither. `out` is device memory: the
// workgroups add to it with atomics.
enum VictimWhy : int32_t {
  kWhyNoPreemptees = 6,
  kWhyNoVictims = 7,
  kWhyNotEnough = 8,
  kWhyVictims = 9,
  kWhyPanic = 10,
  kWhyCauses = 11
};
constexpr int kVictimWhyOut = 2 * kWhyCauses + 3;
struct VictimWhyArgs {
  const VictimScan* q;  // [nq] staged in device memory
  int32_t nq;
  int32_t n_nodes, W, node_lo, node_n;                  // as every query's
  const uint64_t *sel_ok, *taint_ok, *unsched, *live;  // StagePlanes
  int32_t* out;                                         // [nq][kVictimWhyOut]
};
hipError_t launch_victim_why(const VictimWhyArgs& a, const VictimTables& t, hipStream_t stream,
                             hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
hipError_t launch_victim_why_big(const VictimWhyArgs& a, const VictimTables& t, const int32_t* rows, int32_t n_rows,
                                 hipStream_t stream);

// Why a Pending task would not be placed now (kbg_task_reasons). For each of
// n_shapes shapes (a static class, the BestEffort flag and a request) every
// node of the table range [tab_lo, tab_lo + tab_n) whose `live` bit is set goes
// under exactly one cause, the first that applies (allocate.go:119-162,
// backfill.go:50-64); a node whose `live` bit is clear, and a bit of the last
// word at or past tab_lo + tab_n, is counted nowhere whatever the planes hold:
//   cap_check: ntasks >= maxtasks -> 0 (pod cap), sel_ok clear -> 1,
//     unsched set -> 3, taint_ok clear -> 4 (KBG_WHY_* codes; cap_check 0: the
//     predicates plugin is off and none of these occurs);
//   the shape is BestEffort, or req LessEqual Idle       -> kTwhyFitsIdle;
//   req LessEqual Releasing                              -> kTwhyFitsReleasing;
//   otherwise                                            -> kTwhyShort.
// LessEqual is the reference's `r < a || |a - r| < min` per dimension. Host
// ports (2), pod affinity (5) and a nil Node (kTwhyPanic) are the host's:
// sessions holding any take the host path for the whole table.
// Row s of `out` (kTaskWhyOut words): count[kTwhyCauses], first_node
// [kTwhyCauses] (lowest global node of the cause, -1 none), idle_short[3]: over
// the nodes of kTwhyFitsReleasing and kTwhyShort, the dimensions (cpu, memory,
// GPU) in which Idle.FitDelta(req) is negative, kbg_fitdelta_kernel's
// expression (a dimension of request 0 subtracts nothing); one word of padding.
// launch_task_why_init sets every row to its empty value; launch_task_why,
// after it on the same stream, adds the table's nodes. `out` is device memory:
// the workgroups add to it with atomics. tab_lo is a multiple of 64.
enum TaskWhy : int32_t { kTwhyFitsIdle = 6, kTwhyFitsReleasing = 7, kTwhyShort = 8, kTwhyPanic = 9, kTwhyCauses = 10 };
constexpr int kTaskWhyOut = 2 * kTwhyCauses + 4;
constexpr int kTaskWhyGroup = 16;  // shapes per workgroup
constexpr int kTaskWhyWaves = 4;   // 64-node words per workgroup, one per wave
constexpr int32_t kTaskShapeBestEffort = 1;
struct TaskShape {
  int32_t cls;
  int32_t flags;  // kTaskShapeBestEffort: Resreq.IsEmpty(), no resource test
  double req[3];
};
struct TaskWhyArgs {
  const double* nodes;  // the node table block (FirstFitArgs.nodes)
  int32_t stride, W, tab_lo, tab_n;
  const uint64_t *sel_ok, *taint_ok, *unsched, *live;  // StagePlanes
  const TaskShape* shapes;                             // [n_shapes] staged in device memory
  int32_t n_shapes, cap_check;
  int32_t* out;  // [n_shapes][kTaskWhyOut]
};
hipError_t launch_task_why_init(int32_t* out, int32_t n_shapes, hipStream_t stream);
hipError_t launch_task_why(const TaskWhyArgs& a, hipStream_t stream, hipEvent_t start = nullptr,
                           hipEvent_t stop = nullptr);

// How many copies of a Pending task fit now (kbg_task_headroom). For each of
// n_shapes shapes (TaskShape, as above) and every node n of the table range
// whose `live` bit is set and which passes the static stages exactly as in
// launch_task_why (cap_check: ntasks < maxtasks, sel_ok set, unsched clear,
// taint_ok set; cap_check 0: every live node passes), with `limit` in
// [1, kRoomMaxLimit] the same for the whole launch:
//   room  = cap_check ? maxtasks[n] - ntasks[n] : INT32_MAX      (> 0 here)
//   bound = min(limit, room)
//   i = 0; a = Idle[n];      while (i < bound && LE(req, a)) { a -= req; ++i; }   k_idle = i
//          b = Releasing[n]; while (i < bound && LE(req, b)) { b -= req; ++i; }   k_rel  = i - k_idle
// the copies allocate would put on the node one after the other
// (allocate.go:119-162: LessEqual(Idle) then Idle.Sub, else LessEqual
// (Releasing) then Releasing.Sub, node_info.go:101-129), under the pod cap of
// predicates.go:125-127. LE is the reference's `r < x || |x - r| < min` per
// dimension and the subtraction plain fp64 per dimension, one copy at a time:
// the iteration is the definition (a request dimension below its min keeps
// fitting while Idle drifts negative; a - k * req is not the iterated value).
// A BestEffort shape takes no resource test (backfill.go:47-60): k_idle =
// bound, k_rel = 0.
// Row s of `out` (kRoomOut words), over those nodes:
//   kRoomCopiesIdle       sum of k_idle
//   kRoomCopiesRel        sum of k_rel
//   kRoomNodesIdle        nodes with k_idle > 0
//   kRoomNodesRelOnly     nodes with k_idle == 0 && k_rel > 0
//   kRoomFirstNode        lowest global node with k_idle + k_rel > 0, -1 none
//   kRoomMaxNodeCopies    max of k_idle + k_rel
//   kRoomNodesPass        the nodes past the stages
//   kRoomLimitHit         nodes with k_idle + k_rel == limit and limit < room:
//                         their count may have been cut, the sums are lower bounds
// launch_task_headroom_init sets every row to its empty value;
// launch_task_headroom, after it on the same stream, adds the table's nodes
// with integer atomics. tab_lo is a multiple of 64. The launcher refuses
// (hipErrorInvalidValue, nothing launched) a limit outside [1, kRoomMaxLimit]
// and tab_n * limit > INT32_MAX, so no sum can wrap.
enum TaskRoom : int32_t {
  kRoomCopiesIdle = 0,
  kRoomCopiesRel = 1,
  kRoomNodesIdle = 2,
  kRoomNodesRelOnly = 3,
  kRoomFirstNode = 4,
  kRoomMaxNodeCopies = 5,
  kRoomNodesPass = 6,
  kRoomLimitHit = 7,
  kRoomOut = 8
};
constexpr int32_t kRoomMaxLimit = 1024;
constexpr int kRoomBits = 11;  // k_idle, k_rel <= kRoomMaxLimit = 2^10
struct TaskRoomArgs {
  const double* nodes;  // the node table block (FirstFitArgs.nodes)
  int32_t stride, W, tab_lo, tab_n;
  const uint64_t *sel_ok, *taint_ok, *unsched, *live;  // StagePlanes
  const TaskShape* shapes;                             // [n_shapes] staged in device memory
  int32_t n_shapes, cap_check, limit;
  int32_t* out;  // [n_shapes][kRoomOut]
};
hipError_t launch_task_headroom_init(int32_t* out, int32_t n_shapes, hipStream_t stream);
hipError_t launch_task_headroom(const TaskRoomArgs& a, hipStream_t stream, hipEvent_t start = nullptr,
                                hipEvent_t stop = nullptr);

// Where a job's Pending tasks would land now (kbg_job_fit). Each of n_jobs
// jobs is a walk of steps job_off[j] .. job_off[j + 1], at most kFitMaxSteps,
// taken in order against a view of the table range that is private to the job
// and starts as the table is. A step is a shape (TaskShape, never BestEffort).
// It goes to the lowest node of the range whose `live` bit is set, which
// passes the static stages against the view as in launch_task_headroom
// (cap_check: ntasks < maxtasks, sel_ok set, unsched clear, taint_ok set;
// cap_check 0: every live node passes) and on which
//   LE(req, Idle)        -> kind 0 (Allocate):  Idle -= req, ntasks += 1
//   else LE(req, Releasing) -> kind 1 (Pipeline): Releasing -= req, ntasks += 1
// (allocate.go:119-162: the Releasing test of a node comes before the Idle
// test of the next; node_info.go:101-129). LE is the reference's
// `r < x || |x - r| < min` per dimension, the subtraction plain fp64. A step
// no node takes leaves the view as it is, and the walk goes on
// (allocate.go:170). out[2 * step] is the global node or -1, out[2 * step + 1]
// the kind (0 with node -1).
// `prev` is the index within the job's walk of the previous step of the same
// shape, or -1: the scan starts at the node that step landed on, inclusive,
// and a step whose prev landed nowhere lands nowhere without a scan. Inside a
// walk the view only loses Idle and Releasing and only gains pods, so with a
// request without a negative dimension a node that turned a shape away keeps
// turning it away: the cursor changes no result. A shape with a negative
// request dimension must come with prev = -1 on every step.
// The node table and the planes are read only. h_shapes, h_steps and h_job_off
// are the host's copies of the three staged arrays: the launcher reads them
// and refuses (hipErrorInvalidValue, nothing launched) a job of more than
// kFitMaxSteps steps, a shape index outside n_shapes, a BestEffort shape, a
// prev that is not an earlier step of the same job and shape, and a table
// range of more than kFitMaxNodes nodes (the kernel's touched-word bitmap).
// n_jobs <= 0 or tab_n <= 0 is a successful no-op.
constexpr int32_t kFitMaxSteps = 512;
constexpr int32_t kFitMaxNodes = 1 << 20;
struct JobFitStep {
  int32_t shape, prev;
};
struct JobFitArgs {
  const double* nodes;  // the node table block (FirstFitArgs.nodes)
  int32_t stride, W, tab_lo, tab_n;
  const uint64_t *sel_ok, *taint_ok, *unsched, *live;  // StagePlanes
  const TaskShape* shapes;                             // [n_shapes] staged in device memory
  const JobFitStep* steps;                             // [job_off[n_jobs]] staged in device memory
  const int32_t* job_off;                              // [n_jobs + 1] staged in device memory
  int32_t n_shapes, n_jobs, cap_check;
  int32_t* out;  // [job_off[n_jobs]][2]
  const TaskShape* h_shapes;
  const JobFitStep* h_steps;
  const int32_t* h_job_off;
};
// What launch_job_fit refuses, named; nullptr for a legal launch.
inline const char* job_fit_refusal(const JobFitArgs& a) {
  if (a.tab_n > kFitMaxNodes) return "table range past the touched-word bitmap";
  if (a.n_jobs <= 0 || a.tab_n <= 0) return nullptr;
  if (!a.h_shapes || !a.h_steps || !a.h_job_off) return "null host copy";
  if (a.h_job_off[0] != 0) return "job_off does not start at 0";
  for (int32_t j = 0; j < a.n_jobs; ++j) {
    const int32_t s0 = a.h_job_off[j], ns = a.h_job_off[j + 1] - s0;
    if (ns < 0) return "job_off descends";
    if (ns > kFitMaxSteps) return "a job of more than 512 steps";
    for (int32_t i = 0; i < ns; ++i) {
      const JobFitStep& st = a.h_steps[s0 + i];
      if (st.shape < 0 || st.shape >= a.n_shapes) return "shape index outside n_shapes";
      if (a.h_shapes[st.shape].flags & kTaskShapeBestEffort) return "a BestEffort shape";
      if (st.prev < -1 || st.prev >= i || (st.prev >= 0 && a.h_steps[s0 + st.prev].shape != st.shape))
        return "prev is not an earlier step of the same job and shape";
    }
  }
  return nullptr;
}
hipError_t launch_job_fit(const JobFitArgs& a, hipStream_t stream, hipEvent_t start = nullptr,
                          hipEvent_t stop = nullptr);

// Which Pending tasks a node would take now (kbg_node_reasons): the table of
// launch_task_why, (live node x shape) -> cause, reduced along the shape axis
// with a weight per shape. A shape record is a TaskShape with the number of
// Pending tasks of that key (`weight` >= 1), those of them whose queue is not
// overused (0 <= weight_open <= weight) and the lowest task index of the key
// (`first_task` >= 0). The causes, cap_check and LessEqual are launch_task_why's
// to the letter; host ports, pod affinity and a nil Node are the host's.
// `words` lists n_words words of the table, ascending and without repeats:
// entry i names the table rows [64 * words[i], 64 * words[i] + 64), the global
// nodes tab_lo + row. Only they are evaluated. `out` holds kNodeWhyFields
// planes of `ostride` >= 64 * n_words words each, field-major, so the 64 lanes
// of a wave store to 64 consecutive words of a plane: the slot of lane l of
// entry i is 64 * i + l in every plane. The planes of a slot:
//   kNwhyCount + k       tasks (sum of weight) under cause kNodeWhyCause[k]
//   kNwhyFirst + k       lowest first_task under that cause, -1 none
//   kNwhyShort + d       over causes 7 and 8: sum of weight where
//                        Idle.FitDelta(req) is negative in cpu, memory, GPU
//   kNwhyOpenIdle        sum of weight_open under kTwhyFitsIdle
//   kNwhyOpenRel         sum of weight_open under kTwhyFitsReleasing
//   kNwhyIdleBestEffort  sum of weight of BestEffort shapes under kTwhyFitsIdle
// launch_node_why_init sets the slots [0, 64 * n_words) of every plane to their
// empty value and nothing else; launch_node_why, after it on the same stream
// and any number of times with further shapes, adds to the slots of live nodes
// inside the table with integer atomics (add, and unsigned min with -1 the
// empty value): the order of shape groups and launches is nothing. A slot of a
// dead node, or of a row at or past tab_n, keeps its empty value; the words of
// a plane from 64 * n_words on are never written. The sum of all weights must
// not pass INT32_MAX (the session's task count bounds it). tab_lo is a multiple
// of 64. The node table and the planes are read only.
constexpr int kNodeWhyGroup = 32;  // shape records per workgroup
constexpr int kNodeWhyWaves = 4;   // list entries per workgroup, one per wave
constexpr int kNodeWhyCauses = 7;  // the device's causes
constexpr int32_t kNodeWhyCause[kNodeWhyCauses] = {0, 1, 3, 4, kTwhyFitsIdle, kTwhyFitsReleasing, kTwhyShort};
enum NodeWhy : int32_t {
  kNwhyCount = 0,
  kNwhyFirst = kNodeWhyCauses,
  kNwhyShort = 2 * kNodeWhyCauses,
  kNwhyOpenIdle = 2 * kNodeWhyCauses + 3,
  kNwhyOpenRel = 2 * kNodeWhyCauses + 4,
  kNwhyIdleBestEffort = 2 * kNodeWhyCauses + 5,
  kNodeWhyFields = 2 * kNodeWhyCauses + 6
};
struct NodeWhyShape {
  TaskShape sh;
  int32_t weight, weight_open, first_task, pad;
};
struct NodeWhyArgs {
  const double* nodes;  // the node table block (FirstFitArgs.nodes)
  int32_t stride, W, tab_lo, tab_n;
  const uint64_t *sel_ok, *taint_ok, *unsched, *live;  // StagePlanes
  const NodeWhyShape* shapes;                          // [n_shapes] staged in device memory
  int32_t n_shapes, cap_check;
  const int32_t* words;  // [n_words] staged in device memory
  int32_t n_words;
  int32_t ostride;
  int32_t* out;  // [kNodeWhyFields][ostride]
};
hipError_t launch_node_why_init(int32_t* out, int32_t ostride, int32_t n_words, hipStream_t stream);
hipError_t launch_node_why(const NodeWhyArgs& a, hipStream_t stream, hipEvent_t start = nullptr,
                           hipEvent_t stop = nullptr);

// Where a node's running pods would land if it left (kbg_node_drain). Each of
// n_walks walks is launch_job_fit's walk (the view, the stages, LE, the
// subtraction, `prev`, `out`, tab_lo a multiple of 64: all as JobFitArgs says)
// with three differences.
// - Exclusion. walk_row[w] is the table row (node - tab_lo) that takes nothing
//   in walk w: the drained node. A row outside [0, tab_n) excludes nothing (the
//   node belongs to another range), and -1 is the way to say so. `excl` is one
//   plane of W words over the global nodes, common to the launch: a set bit
//   takes nothing in any walk (the cordon). Both hold with cap_check 0. They
//   are and-ed out of the word's `valid` as `live` is and-ed in, so an excluded
//   node is never a candidate and never enters the view.
// - BestEffort. A shape with kTaskShapeBestEffort goes to the lowest node that
//   passes the stages, with no resource test (backfill.go:47-64): kind 0,
//   ntasks += 1, Idle -= req (Resreq.IsEmpty(): every dimension below its min,
//   mostly zero; node_info.go:108-118 subtracts it all the same).
// - The steps of a walk may be of any mix of shapes and classes: that is what
//   a drain is. The cursor is job fit's: a BestEffort shape keeps it (a view
//   only gains pods), a shape with a negative request dimension never has one.
// h_shapes, h_steps, h_walk_off and h_walk_row are the host's copies of the
// staged arrays. launch_drain refuses (hipErrorInvalidValue, nothing launched)
// what launch_job_fit refuses except a BestEffort shape, and also a walk_row
// below -1 and more than kDrainMaxWalks walks.
// n_walks <= 0 or tab_n <= 0 is a successful no-op.
constexpr int32_t kDrainMaxWalks = 1 << 20;
struct DrainArgs {
  const double* nodes;  // the node table block (FirstFitArgs.nodes)
  int32_t stride, W, tab_lo, tab_n;
  const uint64_t *sel_ok, *taint_ok, *unsched, *live;  // StagePlanes
  const uint64_t* excl;                                // [W] staged in device memory
  const TaskShape* shapes;                             // [n_shapes] staged in device memory
  const JobFitStep* steps;                             // [walk_off[n_walks]] staged in device memory
  const int32_t* walk_off;                             // [n_walks + 1] staged in device memory
  const int32_t* walk_row;                             // [n_walks] staged in device memory
  int32_t n_shapes, n_walks, cap_check;
  int32_t* out;  // [walk_off[n_walks]][2]
  const TaskShape* h_shapes;
  const JobFitStep* h_steps;
  const int32_t* h_walk_off;
  const int32_t* h_walk_row;
};
// What launch_drain refuses, named; nullptr for a legal launch.
inline const char* drain_refusal(const DrainArgs& a) {
  if (a.tab_n > kFitMaxNodes) return "table range past the touched-word bitmap";
  if (a.n_walks > kDrainMaxWalks) return "more than 2^20 walks";
  if (a.n_walks <= 0 || a.tab_n <= 0) return nullptr;
  if (!a.h_shapes || !a.h_steps || !a.h_walk_off || !a.h_walk_row) return "null host copy";
  if (a.h_walk_off[0] != 0) return "walk_off does not start at 0";
  for (int32_t j = 0; j < a.n_walks; ++j) {
    const int32_t s0 = a.h_walk_off[j], ns = a.h_walk_off[j + 1] - s0;
    if (ns < 0) return "walk_off descends";
    if (ns > kFitMaxSteps) return "a walk of more than 512 steps";
    if (a.h_walk_row[j] < -1) return "a drained row below -1";
    for (int32_t i = 0; i < ns; ++i) {
      const JobFitStep& st = a.h_steps[s0 + i];
      if (st.shape < 0 || st.shape >= a.n_shapes) return "shape index outside n_shapes";
      if (st.prev < -1 || st.prev >= i || (st.prev >= 0 && a.h_steps[s0 + st.prev].shape != st.shape))
        return "prev is not an earlier step of the same walk and shape";
    }
  }
  return nullptr;
}
hipError_t launch_drain(const DrainArgs& a, hipStream_t stream, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

}  // namespace kbg
