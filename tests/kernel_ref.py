"""A plain reference of the scan, first-fit, select and FitError kernels
(kube-arbitrator_amd/csrc/kbg_kernels.hip), in numpy and Python integers, and
the comparator of the kernel probes' raw output (tools/kernel_probe.cpp).

Nothing here has a tolerance: every comparison is on integers and exact.
General mode evaluates the reference's own float64 expression
(resource_info.go:142-146); integer mode evaluates it on the original
requests in exact integers (int64: every magnitude is <= 2^52), while the
kernel is given the thresholds req - min in float64 (kbg_svc_link.ipp
Grouper::build), so the equivalence kbg_device.hpp claims for TaskRec is
itself under test."""
from dataclasses import dataclass, field

import numpy as np

# resource_info.go:54-56 (kbg_device.hpp kMinMilliCPU, kMinMemory, kMinMilliGPU)
K_MIN = (10.0, 10.0 * 1024.0 * 1024.0, 10.0)
K_MIN_INT = (10, 10 * 1024 * 1024, 10)
# kbg_device.hpp
CAND_PIPELINE_BIT = 0x80000000
COUNT_INCOMPLETE_BIT = 0x40000000
INFO_ANY_BIT = 0x20000000
INFO_WORDS_MASK = 0x00FFFFFF
ROW_WRITER = 0x80000000
ROW_REL_ZERO_FITS = 1
ROW_WANT_SHIFT = 1
INLINE_SHAPES = 96
FF_ROUND_WORDS = 128
FF_MAX_SPLITS = 8
SCAN_ROWS_PER_BLOCK = 64
# tools/kernel_probe.cpp
SENTINEL = 0xA5
GUARD_BYTES = 4096

TASK_REC = np.dtype([("req", "<f8", (3,)), ("cls", "<i4"), ("flags", "<i4")])
FIT_QUERY = np.dtype([("cls", "<i4"), ("end", "<i4"), ("point", "<i4"), ("win", "<i4"), ("req", "<f8", (3,))])
NODE_DELTA = np.dtype([("node", "<i4"), ("ntasks", "<i4"), ("idle", "<f8", (3,)), ("rel", "<f8", (3,)),
                       ("maxtasks", "<i4"), ("pad", "<i4")])
MASK_DELTA = np.dtype([("index", "<u4"), ("pad", "<u4"), ("value", "<u8")])


def less_equal(r, a, mn):
    """One dimension of Resource.LessEqual in float64: r < a || |a - r| < min."""
    r = np.asarray(r, dtype=np.float64)
    a = np.asarray(a, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        return (r < a) | (np.abs(a - r) < np.float64(mn))


def less_equal_int(r, a, mn):
    """The same on exact integers (int64, or Python integers in object arrays)."""
    return (r < a) | (abs(a - r) < mn)


def threshold(req, mn):
    """The integer-mode row value the host hands the kernel: req - min in float64."""
    return np.float64(req) - np.float64(mn)


def firstfit_geometry(G, full_scan):
    """kbg_kernels.hip firstfit_geometry: (variant, rows per workgroup)."""
    if not full_scan:
        v = 16 if G <= 16 * 256 else 24 if G <= 24 * 256 else 32
        return v, v
    rows = (G + 255) // 256
    rows = min(32, max(2, (rows + 1) & ~1))
    return (16 if rows <= 16 else 24 if rows <= 24 else 32), rows


def pack_words(bits):
    """bool [..., 64 * n] -> uint64 [..., n], bit b of word w = node 64 * w + b."""
    return np.ascontiguousarray(np.packbits(bits, axis=-1, bitorder="little")).view("<u8")


def popcount(words):
    """Set bits of each uint64 word."""
    b = np.unpackbits(np.ascontiguousarray(words).view(np.uint8), axis=-1)
    return b.reshape(words.shape + (64,)).sum(axis=-1, dtype=np.int64)


def sentinel_words(n, dtype):
    return np.frombuffer(bytes([SENTINEL]) * (n * np.dtype(dtype).itemsize), dtype=dtype).copy()


@dataclass
class Table:
    """Node values by global node (W * 64 entries; int64 in integer mode,
    float64 otherwise) and the window [tab_lo, tab_lo + tab_n) the device
    table holds."""
    int_mode: bool
    n_nodes: int
    W: int
    idle: np.ndarray       # [3][W * 64]
    rel: np.ndarray        # [3][W * 64]
    ntasks: np.ndarray     # int32 [W * 64]
    maxtasks: np.ndarray
    class_mask: np.ndarray  # uint64 [classes][W]
    tab_lo: int = 0
    tab_n: int = 0
    stride: int = 0

    def block(self):
        """The device table block (FirstFitArgs.nodes layout): rows of the
        window, then padding rows no legal launch may use (values on which
        every request fits, so a leak shows)."""
        L = self.stride
        f = np.full((6, L), 2.0 ** 52, dtype=np.float64)
        sl = slice(self.tab_lo, self.tab_lo + self.tab_n)
        f[0:3, :self.tab_n] = self.idle[:, sl]
        f[3:6, :self.tab_n] = self.rel[:, sl]
        i = np.zeros((2, L), dtype=np.int32)
        i[1] = 1 << 30
        i[0, :self.tab_n] = self.ntasks[sl]
        i[1, :self.tab_n] = self.maxtasks[sl]
        return f.tobytes() + i.tobytes()


def fit_planes(tab, req, backfill, cls, cap_check, windowed=True):
    """(f, fi) uint64 [W] for one evaluation row: fi = static & valid & pod cap
    & fit(Idle); f = fi | static & valid & cap & fit(Releasing)."""
    n = tab.W * 64
    node = np.arange(n)
    valid = node < tab.n_nodes
    if windowed:
        valid &= (node >= tab.tab_lo) & (node < tab.tab_lo + tab.tab_n)
    static = np.unpackbits(tab.class_mask[cls].view(np.uint8), bitorder="little").astype(bool)
    ok = static & valid
    if cap_check:
        ok &= tab.ntasks < tab.maxtasks
    if backfill:  # PredicateFn only: every node fits
        fi = fr = np.ones(n, dtype=bool)
    else:
        fi = np.ones(n, dtype=bool)
        fr = np.ones(n, dtype=bool)
        for d in range(3):
            if tab.int_mode:
                fi &= less_equal_int(int(req[d]), tab.idle[d], K_MIN_INT[d])
                fr &= less_equal_int(int(req[d]), tab.rel[d], K_MIN_INT[d])
            else:
                fi &= less_equal(req[d], tab.idle[d], K_MIN[d])
                fr &= less_equal(req[d], tab.rel[d], K_MIN[d])
    fi = fi & ok
    return pack_words(fi | (fr & ok)), pack_words(fi)


def rel_zero_fits(int_mode, req, backfill):
    """kRowRelZeroFits: LessEqual(Resreq, 0), as Grouper::build sets it."""
    if backfill:
        return True
    if int_mode:
        return all(less_equal_int(int(req[d]), 0, K_MIN_INT[d]) for d in range(3))
    return all(bool(less_equal(req[d], 0.0, K_MIN[d])) for d in range(3))


def task_records(int_mode, protos, backfill, proto_of, cls, want=None):
    """TaskRec rows: the request (thresholds in integer mode, -inf for
    backfill rows), the class, and flags = rel-zero fit | want << 1."""
    out = np.zeros(len(proto_of), dtype=TASK_REC)
    for i, p in enumerate(proto_of):
        if backfill[p]:
            out["req"][i] = -np.inf
        elif int_mode:
            out["req"][i] = [threshold(int(protos[p][d]), K_MIN_INT[d]) for d in range(3)]
        else:
            out["req"][i] = protos[p]
        fl = ROW_REL_ZERO_FITS if rel_zero_fits(int_mode, protos[p], backfill[p]) else 0
        if want is not None:
            fl |= int(want[i]) << ROW_WANT_SHIFT
        out["flags"][i] = fl
    out["cls"] = cls
    return out


@dataclass
class FfCase:
    """One legal launch of kbg_firstfit_kernel."""
    name: str
    tab: Table
    p: dict                  # the scalar fields of FirstFitArgs (kernel_probe.cpp kbg_probe_ff)
    protos: list             # distinct requests: [3] floats (general) or Python integers
    backfill: list           # per proto: a backfill row (request -inf)
    shape_proto: np.ndarray  # [n_shapes]
    shape_cls: np.ndarray
    shape_want: np.ndarray
    row_shape: np.ndarray = None   # uint32 [G] shape | ROW_WRITER, or None
    run_end: np.ndarray = None     # uint16 [n_shapes] (runs), or None
    claims: set = field(default_factory=set)

    @property
    def int_mode(self):
        return self.tab.int_mode

    def shapes(self):
        return task_records(self.int_mode, self.protos, self.backfill, self.shape_proto, self.shape_cls,
                            self.shape_want)

    def writers(self):
        """bool [n_shapes]: the shape has a writer row."""
        p = self.p
        w = np.zeros(p["n_shapes"], dtype=bool)
        if self.run_end is not None:
            w[:] = True
        elif self.row_shape is not None:
            rs = self.row_shape
            w[(rs[(rs & ROW_WRITER) != 0] & ~np.uint32(ROW_WRITER)).astype(np.int64)] = True
        else:
            w[:p["G"]] = True
        return w

    def parts(self):
        p = self.p
        return [(p["w_lo"] + k * p["split_words"], min(p["w_hi"], p["w_lo"] + (k + 1) * p["split_words"]))
                for k in range(p["splits"])]


def ff_planes(case):
    """(F, FI, inv): planes uint64 [U][W] of the distinct (request, class)
    pairs and each shape's index into them."""
    keys = case.shape_proto.astype(np.int64) * len(case.tab.class_mask) + case.shape_cls
    uniq, inv = np.unique(keys, return_inverse=True)
    F = np.zeros((len(uniq), case.tab.W), dtype=np.uint64)
    FI = np.zeros_like(F)
    nc = len(case.tab.class_mask)
    for u, k in enumerate(uniq):
        pr, cl = int(k) // nc, int(k) % nc
        F[u], FI[u] = fit_planes(case.tab, case.protos[pr], case.backfill[pr], cl, case.p["cap_check"])
    return F, FI, inv


@dataclass
class FfExpected:
    info: np.ndarray      # uint32, guard included
    masks: np.ndarray     # uint64 (f, i interleaved), guard included
    covered: np.ndarray   # [n_shapes][splits], -1 where the shape has no writer
    fits: np.ndarray      # [n_shapes][splits] fits in the part
    F: np.ndarray
    FI: np.ndarray
    inv: np.ndarray


def ff_reference(case):
    """The whole expected `info` and `masks` buffers of the probe: sentinel
    everywhere but the info words and the covered words of writer shapes."""
    p = case.p
    F, FI, inv = ff_planes(case)
    pc = popcount(F)
    ns, mw = p["n_shapes"], p["mw"]
    info = sentinel_words(ns * p["info_stride"] + GUARD_BYTES // 4, "<u4")
    masks = sentinel_words(ns * mw * 2 + GUARD_BYTES // 8, "<u8")
    covered = np.full((ns, p["splits"]), -1, dtype=np.int64)
    fits = np.zeros((ns, p["splits"]), dtype=np.int64)
    writers = case.writers()
    parts = case.parts()
    cum = [np.cumsum(pc[:, lo:hi], axis=1) for lo, hi in parts]
    for s in np.flatnonzero(writers):
        u = inv[s]
        for k, (lo, hi) in enumerate(parts):
            tw = hi - lo
            c = cum[k][u]
            total = int(c[-1])
            if p["complete"]:
                cov = tw
            else:
                want = int(case.shape_want[s])
                # the shortest prefix of the part's words holding at least `want` fits, or all of them
                cov = int(np.searchsorted(c, want, side="left")) + 1 if total >= want else tw
            covered[s, k] = cov
            fits[s, k] = total
            info[s * p["info_stride"] + p["part0"] + k] = (
                cov | (COUNT_INCOMPLETE_BIT if cov < tw else 0) | (INFO_ANY_BIT if total else 0))
            o = (s * mw + lo - p["mask_w0"]) * 2
            masks[o:o + 2 * cov:2] = F[u, lo:lo + cov]
            masks[o + 1:o + 2 * cov:2] = FI[u, lo:lo + cov]
    return FfExpected(info, masks, covered, fits, F, FI, inv)


def ff_compare(case, exp, got_info, got_masks, limit=8):
    """Every difference between the probe's buffers and the expected ones,
    named by shape, part and word: (a) the covered words of writer shapes,
    (b) the info words, (c) the sentinel everywhere else, guards included.
    Returns a list of messages, empty when the buffers are identical."""
    p = case.p
    errs = []
    got_info = np.asarray(got_info, dtype="<u4")
    got_masks = np.asarray(got_masks, dtype="<u8")
    if got_info.shape != exp.info.shape or got_masks.shape != exp.masks.shape:
        return [f"{case.name}: buffer sizes differ"]
    ns, mw, st = p["n_shapes"], p["mw"], p["info_stride"]
    for i in np.flatnonzero(got_info != exp.info)[:limit]:
        i = int(i)
        if i >= ns * st:
            errs.append(f"{case.name}: info guard word {i - ns * st} overwritten: {int(got_info[i]):#x}")
            continue
        s, k = divmod(i, st)
        k -= p["part0"]
        what = "info"
        if 0 <= k < p["splits"] and exp.covered[s, k] >= 0:
            lo, hi = case.parts()[k]
            what = f"info (words [{lo}, {hi}), expected covered through word {lo + int(exp.covered[s, k]) - 1})"
        else:
            what = "info slot no writer owns"
        errs.append(f"{case.name}: shape {s} part {k} {what}: got {int(got_info[i]):#x} expected "
                    f"{int(exp.info[i]):#x}")
    for i in np.flatnonzero(got_masks != exp.masks)[:limit]:
        i = int(i)
        if i >= ns * mw * 2:
            errs.append(f"{case.name}: masks guard word {i - ns * mw * 2} overwritten: {int(got_masks[i]):#x}")
            continue
        s, r = divmod(i, mw * 2)
        w = p["mask_w0"] + r // 2
        plane = "Idle plane" if r & 1 else "fit plane"
        k = (w - p["w_lo"]) // p["split_words"] if p["w_lo"] <= w < p["w_hi"] else -1
        where = "outside [w_lo, w_hi)"
        if k >= 0:
            cov = int(exp.covered[s, k])
            lo = case.parts()[k][0]
            where = ("not a writer shape" if cov < 0 else
                     f"covered (part covers [{lo}, {lo + cov}))" if w < lo + cov else
                     f"past covered (part covers [{lo}, {lo + cov})): sentinel expected")
        errs.append(f"{case.name}: shape {s} word {w} part {k} {plane}, {where}: got {int(got_masks[i]):#018x} "
                    f"expected {int(exp.masks[i]):#018x}")
    return errs


# ----------------------------------------------------------- scan + select
def scan_reference(tab, recs_proto, protos, backfill, cls, cap_check, Wl, slots):
    """The [slot][plane][quad][row][4] bitmap buffer of launch_scan over every
    slot, guard included: words past W and the padding of the last quad keep
    the sentinel. Returns (buffer, F, FI) with F, FI [n_tasks][W]."""
    n = len(recs_proto)
    sw = (Wl + 3) & ~3
    plane = n * sw
    buf = sentinel_words(slots * 2 * plane + GUARD_BYTES // 8, "<u8")
    F = np.zeros((n, tab.W), dtype=np.uint64)
    FI = np.zeros_like(F)
    memo = {}
    for t in range(n):
        key = (int(recs_proto[t]), int(cls[t]))
        if key not in memo:
            memo[key] = fit_planes(tab, protos[key[0]], backfill[key[0]], key[1], cap_check, windowed=False)
        F[t], FI[t] = memo[key]
    rows = np.arange(n)
    for c in range(min(tab.W, slots * Wl)):
        slot, w = divmod(c, Wl)
        o = slot * 2 * plane + ((w >> 2) * n + rows) * 4 + (w & 3)
        buf[o] = F[:, c]
        buf[o + plane] = FI[:, c]
    return buf, F, FI


def select_reference(F, FI, w_lo, w_hi, cap_off):
    """launch_select: per row the first M fits in node order over the words
    [w_lo, w_hi), kCandPipelineBit where the Idle plane is clear; the count,
    with kCountIncompleteBit when fits remain. Buffers with guards."""
    n = len(F)
    cand = sentinel_words(int(cap_off[n]) + GUARD_BYTES // 4, "<u4")
    count = sentinel_words(n + GUARD_BYTES // 4, "<u4")
    for t in range(n):
        M = int(cap_off[t + 1] - cap_off[t])
        f = np.unpackbits(F[t, w_lo:w_hi].view(np.uint8), bitorder="little")
        fi = np.unpackbits(FI[t, w_lo:w_hi].view(np.uint8), bitorder="little")
        nodes = np.flatnonzero(f)
        take = nodes[:M]
        vals = (take + w_lo * 64).astype(np.uint32) | np.where(fi[take] != 0, 0, CAND_PIPELINE_BIT).astype(np.uint32)
        cand[int(cap_off[t]):int(cap_off[t]) + len(take)] = vals
        count[t] = len(take) | (COUNT_INCOMPLETE_BIT if len(nodes) > M else 0)
    return cand, count


# ---------------------------------------------------------------- FitError
def _le3(req, c, m, g):
    return bool(less_equal(req[0], c, K_MIN[0]) and less_equal(req[1], m, K_MIN[1]) and less_equal(req[2], g, K_MIN[2]))


def fitdelta_reference(tab, hoff, hk, hold, queries, cap_check):
    """kbg_fitdelta_kernel (kbg_kernels.hip "FitError counts"), restated as a
    direct loop: per query, over the nodes [tab_lo, min(end, tab_lo + tab_n))
    that pass the static predicate, the node's state at the query's point
    (the decisions at or after `point` undone: the Idle before the first
    undone Allocate, the pod count less the undone decisions); a node that is
    neither capped nor chosen counts as an entry, with Resource.FitDelta's
    negative dimensions (+min only where the request is positive)."""
    out = sentinel_words(len(queries) * 4 + GUARD_BYTES // 4, "<i4")
    for qi, q in enumerate(queries):
        cnt = [0, 0, 0, 0]
        req = [float(x) for x in q["req"]]
        end = min(int(q["end"]), tab.tab_lo + tab.tab_n)
        for n in range(tab.tab_lo, end):
            if not (int(tab.class_mask[int(q["cls"]), n >> 6]) >> (n & 63)) & 1:
                continue
            e0, e1 = int(hoff[n]), int(hoff[n + 1])
            undone = [e for e in range(e0, e1) if (int(hk[e]) & 0x7FFFFFFF) >= int(q["point"])]
            c, m, g = (float(tab.idle[d][n]) for d in range(3))
            for e in undone:
                if not int(hk[e]) & 0x80000000:  # the first undone Allocate: Idle before it
                    c, m, g = (float(x) for x in hold[e])
                    break
            capped = bool(cap_check) and int(tab.ntasks[n]) - len(undone) >= int(tab.maxtasks[n])
            chosen = n != int(q["win"]) and _le3(req, c, m, g)
            if capped or chosen:
                continue
            cnt[0] += 1
            for d, (a, mn) in enumerate(zip((c, m, g), K_MIN)):
                delta = a - (req[d] + mn) if req[d] > 0 else a
                cnt[1 + d] += delta < 0
        out[4 * qi:4 * qi + 4] = cnt
    return out
