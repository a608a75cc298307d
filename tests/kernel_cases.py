"""Seeded inputs of the kernel probes (tests/test_kernels_gpu.py) and what
each first-fit case claims to contain (tests/test_kernel_ref.py checks the
claims on the reference alone, so the matrix cannot pass vacuously).

Node values and requests come from small pools built around each other, so
every table holds the LessEqual tolerance edges: in general mode a - r equal
to +-min and one ulp either side of it, r one ulp either side of a,
fractional values, 0.0 and -0.0; in integer mode a equal to req - min,
req - min + 1 and req, with one request per dimension near 2^51."""
import functools

import numpy as np

import kernel_ref as kr

CLASSES = 3  # class 0 dense, class 1 half, class 2 no node (its shapes fit nowhere)


def value_pools(int_mode):
    """Per dimension: the requests and the node values around them."""
    if int_mode:
        reqs = [[0, 3, 2000, 2 ** 51 - 1000], [0, 1_000_000, 4 << 30, 2 ** 51 - (1 << 30)], [0, 3, 4, 2 ** 51 - 1000]]
        pools = []
        for d, qs in enumerate(reqs):
            mn = kr.K_MIN_INT[d]
            vals = {0, 1}
            for q in qs:
                vals |= {v for v in (q - mn, q - mn + 1, q - 1, q, q + 1, q + mn) if v >= 0}
            pools.append(np.array(sorted(vals), dtype=np.int64))
        return reqs, pools
    reqs = [[0.0, -0.0, 3.0, 2000.5, 64000.0], [0.0, 1.0e6, 4.0 * 2 ** 30, 0.3 * 2 ** 30], [0.0, 3.0, 4.0, 7.25]]
    pools = []
    for d, qs in enumerate(reqs):
        mn = kr.K_MIN[d]
        vals = [0.0, -0.0]
        for q in qs:
            for v in (q - mn, q, q + mn):
                vals += [v, np.nextafter(v, -np.inf), np.nextafter(v, np.inf)]
        pools.append(np.array(vals, dtype=np.float64))
    return reqs, pools


def make_protos(rng, int_mode, n=12):
    """Distinct requests: all zero (Releasing-zero fit), within tolerance of
    zero (the same), a backfill row (-inf), then random combinations."""
    reqs, _ = value_pools(int_mode)
    protos = [[reqs[0][0], reqs[1][0], reqs[2][0]], [reqs[0][2 if not int_mode else 1], reqs[1][1], reqs[2][1]],
              [reqs[0][0], reqs[1][0], reqs[2][0]]]
    if not int_mode:
        protos[0][0] = -0.0
    backfill = [False, False, True]
    while len(protos) < n:
        protos.append([reqs[d][int(rng.integers(len(reqs[d])))] for d in range(3)])
        backfill.append(False)
    return protos, backfill


def make_table(rng, int_mode, W, n_nodes, rel_mode="some", window=None):
    _, pools = value_pools(int_mode)
    n = W * 64
    dt = np.int64 if int_mode else np.float64
    idle = np.stack([rng.choice(pools[d], size=n) for d in range(3)]).astype(dt)
    rel = np.zeros((3, n), dtype=dt)
    if rel_mode == "some":
        # nonzero Releasing on three nodes of every third word (a single word: of that one); half of
        # them with an Idle nothing fits, so their fits are Releasing-only
        for w in range(W - 1 if W > 1 else 0, -1, -3):
            for lane in rng.choice(64, size=3, replace=False):
                node = w * 64 + int(lane)
                for d in range(3):
                    rel[d, node] = rng.choice(pools[d][pools[d] > 0])
                    if lane & 1:
                        idle[d, node] = 0
    ntasks = rng.integers(0, 4, size=n).astype(np.int32)
    ntasks[(rel != 0).any(axis=0)] = 0  # (the Releasing nodes are below their pod cap)
    maxtasks = rng.integers(1, 4, size=n).astype(np.int32)  # equal to, below and above ntasks
    bits = np.stack([rng.random(n) < 0.9, rng.random(n) < 0.5, np.zeros(n, dtype=bool)])
    bits[:, n_nodes:] = True  # garbage past n_nodes: the kernel must mask it
    tab = kr.Table(int_mode, n_nodes, W, idle, rel, ntasks, maxtasks, kr.pack_words(bits))
    tab.tab_lo, tab.tab_n = window if window else (0, n_nodes)
    tab.stride = (tab.tab_n + 1) // 2 * 2 + 2
    return tab


_WANT_K = (1, 17, 63, 64, 65, 100, 127, 128, 129, 150, 200, 10 ** 6)


def make_ff_case(name, seed, int_mode, tw, G, *, ragged=False, full_scan=False, early_exit=None, addressing="direct",
                 n_shapes=None, splits=1, part0=0, info_extra=0, mask_w0_zero=False, window=False, inner=False,
                 rel_mode="some", cap_check=1):
    rng = np.random.default_rng(seed)
    W = tw + (3 if inner else 0)
    w_lo = 1 if inner else 0
    w_hi = w_lo + tw
    n_nodes = 64 * W - (37 if ragged else 0)
    win = None
    if window:  # the first and the last word of the walk partly outside the table window
        lo = 64 * w_lo + 13
        win = (lo, min(n_nodes, 64 * w_hi) - 20 - lo)
    tab = make_table(rng, int_mode, W, n_nodes, rel_mode, win)
    protos, backfill = make_protos(rng, int_mode)
    if early_exit is None:
        early_exit = 0 if full_scan else 1
    complete = 1 if tw <= kr.FF_ROUND_WORDS else 0
    row_shape = run_end = None
    if addressing == "direct":
        n_shapes = G if n_shapes is None else n_shapes
    elif addressing == "row_shape":
        n_shapes = max(1, G // 3) if n_shapes is None else n_shapes
        # rows of a shape interleaved with the others', the shape's last row its writer; with four or
        # more shapes the last one has no row, so its slots must keep the sentinel
        owned = n_shapes - 1 if n_shapes >= 4 else n_shapes
        rs = np.concatenate([np.arange(min(owned, G)), rng.integers(0, owned, size=max(0, G - owned))])
        rs = rng.permutation(rs).astype(np.uint32)
        last = {int(s): g for g, s in enumerate(rs)}
        for s, g in last.items():
            rs[g] |= np.uint32(kr.ROW_WRITER)
        row_shape = rs
    else:  # runs
        n_shapes = min(kr.INLINE_SHAPES, max(1, G // 3)) if n_shapes is None else n_shapes
        cuts = np.sort(rng.choice(np.arange(1, G), size=n_shapes - 1, replace=False)) if n_shapes > 1 else []
        run_end = np.concatenate([cuts, [G]]).astype(np.uint16)
    shape_proto = rng.integers(0, len(protos), size=n_shapes)
    shape_cls = rng.integers(0, 2, size=n_shapes)
    if n_shapes >= 3:
        shape_cls[1] = 2  # fits nowhere
        shape_proto[0], shape_proto[2] = 1, 2  # Releasing-zero fit, backfill
    split_words = (tw + splits - 1) // splits
    assert (splits - 1) * split_words < tw, "an empty part"
    mask_w0 = 0 if mask_w0_zero else w_lo
    p = dict(G=G, n_shapes=n_shapes, mw=w_hi - mask_w0 + 2, n_nodes=n_nodes, W=W, w_lo=w_lo, w_hi=w_hi,
             tab_lo=tab.tab_lo, tab_n=tab.tab_n, cap_check=cap_check, early_exit=early_exit, complete=complete,
             splits=splits, split_words=split_words, rows=kr.firstfit_geometry(G, not early_exit)[1],
             info_stride=part0 + splits + info_extra, part0=part0, mask_w0=mask_w0,
             runs=1 if run_end is not None else 0, stride=tab.stride, classes=CLASSES, int_mode=1 if int_mode else 0)
    case = kr.FfCase(name, tab, p, protos, backfill, shape_proto, shape_cls, np.ones(n_shapes, dtype=np.int64),
                     row_shape, run_end)
    # want, from the fits of the walk's words: 1; exactly the fits of the first k words, that +-1; more
    # than all fits; k in the first 64-word chunk, the second one and a later round
    F, _, inv = kr.ff_planes(case)
    cum = np.cumsum(kr.popcount(F[:, w_lo:w_hi]), axis=1)
    for s in range(n_shapes):
        c = cum[inv[s]]
        k = min(_WANT_K[(s // 6) % len(_WANT_K)], tw)
        case.shape_want[s] = max(1, (1, int(c[k - 1]), int(c[k - 1]) - 1, int(c[k - 1]) + 1, int(c[-1]) + 5,
                                     int(c[min(tw, 64 + s % 60 + 1) - 1]))[s % 6])
    case.claims = {"nofit", "last_word_fit"} if n_shapes >= 3 else set()
    if not complete and n_shapes >= 8:
        case.claims |= {"cut", "uncut"}
    if rel_mode == "some":
        case.claims.add("rel_only")
        if tw >= 3 and not window:
            case.claims.add("rel_words")
    if ragged and not inner:
        case.claims.add("garbage_mask")
    return case


def check_claims(case, exp):
    """What the case claims, asserted on the reference alone."""
    p, tab = case.p, case.tab
    wr = case.writers()
    lo, hi = p["w_lo"], p["w_hi"]
    F, FI = exp.F[exp.inv][:, lo:hi], exp.FI[exp.inv][:, lo:hi]
    tws = np.array([b - a for a, b in case.parts()])
    if "cut" in case.claims:
        assert ((exp.covered < tws) & wr[:, None]).any(), "no cut list"
    if "uncut" in case.claims:
        assert ((exp.covered == tws) & wr[:, None]).any(), "no uncut list"
    if "nofit" in case.claims:
        assert (wr & (exp.fits.sum(axis=1) == 0)).any(), "no writer shape without a fit"
        assert (wr & (exp.fits.sum(axis=1) > 0)).any(), "no writer shape with a fit"
    if "last_word_fit" in case.claims:
        assert (F[wr][:, -1] != 0).any(), "no fit in the last word"
    if "rel_only" in case.claims:
        assert ((F[wr] & ~FI[wr]) != 0).any(), "no Releasing-only fit"
    if "rel_words" in case.claims:
        node = np.arange(tab.W * 64)
        valid = (node < tab.n_nodes) & (node >= tab.tab_lo) & (node < tab.tab_lo + tab.tab_n)
        nz = ((tab.rel != 0).any(axis=0) & valid).reshape(tab.W, 64).any(axis=1)[lo:hi]
        assert nz.any() and not nz.all(), "Releasing is not nonzero on some words only"
    if "garbage_mask" in case.claims:
        assert hi == tab.W and tab.n_nodes % 64
        past = ~np.uint64(0) << np.uint64(tab.n_nodes % 64)
        used = np.unique(case.shape_cls[wr])
        assert all(int(tab.class_mask[c, -1] & past) for c in used), "no class-mask bit past n_nodes"


# seeds picked where the running one misses a claim (a single word whose Releasing nodes nothing fits)
_SEEDS = {"words1-int": 2007}


def ff_cases():
    """The first-fit matrix, each case in integer and in general mode."""
    out = []
    seed = [1000]

    def add(name, tw, G, **kw):
        for int_mode in (True, False):
            seed[0] += 1
            full = f"{name}-{'int' if int_mode else 'gen'}"
            out.append((full, _SEEDS.get(full, seed[0]), int_mode, tw, G, kw))

    # word counts: one round stored as scanned (complete), then rounds of 128 with the extraction
    for tw in (1, 15, 16, 17, 33, 64, 65, 79, 128):
        for ragged in (False, True):
            add(f"words{tw}{'r' if ragged else ''}", tw, 40, ragged=ragged, cap_check=tw & 1)
    for tw in (129, 130, 192, 257, 300):
        for ee in (0, 1):
            for ragged in (False, True):
                add(f"words{tw}{'r' if ragged else ''}-ee{ee}", tw, 40, ragged=ragged, early_exit=ee,
                    cap_check=tw & 1)
    # row geometry: the 16-, 24- and 32-row variants, grouped (whole blocks) and full-scan (rows spread
    # over the CUs: nrows < ROWS), each at a complete and a multi-round word count
    for tw in (17, 130):
        for G in (1, 15, 16, 17, 40, 4100, 6200):
            add(f"rows{G}-w{tw}", tw, G, ragged=True)
        for G in (600, 4300, 7000):
            add(f"fullscan{G}-w{tw}", tw, G, ragged=True, full_scan=True, addressing="row_shape", n_shapes=G // 5)
    # shape addressing: the row is the shape; a row -> shape map; run ends; 96 shapes inline, 97 host-mapped
    for tw in (33, 192):
        add(f"direct96-w{tw}", tw, 96)
        add(f"direct97-w{tw}", tw, 97)
        add(f"rowshape-w{tw}", tw, 300, full_scan=True, addressing="row_shape", n_shapes=97)
        add(f"rowshape-inline-w{tw}", tw, 90, full_scan=True, addressing="row_shape", n_shapes=30)
        add(f"runs-w{tw}", tw, 300, full_scan=True, addressing="runs", n_shapes=96)
        add(f"runs-short-w{tw}", tw, 37, full_scan=True, addressing="runs", n_shapes=9)
    # splits with a short last part, info words of other ranks around this launch's, masks from word 0
    for splits in (1, 2, 3, 8):
        add(f"splits{splits}-w79", 79, 40, ragged=True, splits=splits, part0=splits & 1, info_extra=2,
            mask_w0_zero=bool(splits & 2), inner=bool(splits & 2))
        add(f"splits{splits}-w300", 300, 40, splits=splits, part0=2, info_extra=1,
            mask_w0_zero=not splits & 2, inner=not splits & 2)
    # a table window smaller than the table, the walk strictly inside W
    for tw in (40, 140):
        add(f"window-w{tw}", tw, 40, window=True, inner=True)
        add(f"window-edge-w{tw}", tw, 40, window=True, ragged=True, mask_w0_zero=True)
    # Releasing zero everywhere (every wave takes the shortcut) against some words only; the pod cap off
    for tw in (20, 150):
        add(f"relzero-w{tw}", tw, 40, rel_mode="zero")
        add(f"nocap-w{tw}", tw, 40, cap_check=0, ragged=True)
    return out


@functools.lru_cache(maxsize=None)
def ff_case(name):
    for n, seed, int_mode, tw, G, kw in ff_cases():
        if n == name:
            return make_ff_case(n, seed, int_mode, tw, G, **kw)
    raise KeyError(name)


FF_NAMES = [c[0] for c in ff_cases()]


def instantiation(case):
    """(mode, walk, ROWS) of the kbg_firstfit_kernel instantiation the case launches."""
    p = case.p
    walk = "complete" if p["complete"] else "early-exit" if p["early_exit"] else "full-scan"
    return ("int" if p["int_mode"] else "general", walk, kr.firstfit_geometry(p["G"], not p["early_exit"])[0])


# ----------------------------------------------------------- scan + select
SCAN_CASES = {
    # name: (n_tasks, Wl, slots, W, w_lo, w_hi)
    "t16-1slot": (16, 5, 1, 5, 0, 5),
    "t17-3slots": (17, 7, 3, 19, 0, 19),        # Wl no multiple of 4, the last slot partly past W
    "t64-3slots-inner": (64, 7, 3, 19, 2, 17),
    "t1024-1slot": (1024, 9, 1, 9, 0, 9),       # the last batch size on 16-row workgroups
    "t1025-3slots": (1025, 6, 3, 17, 0, 17),    # 64-row workgroups
    "t17-2chunks": (17, 70, 1, 70, 0, 70),      # the select's second 64-word chunk
}


@functools.lru_cache(maxsize=None)
def scan_case(name, int_mode):
    n_tasks, Wl, slots, W, w_lo, w_hi = SCAN_CASES[name]
    rng = np.random.default_rng(7000 + sorted(SCAN_CASES).index(name) * 2 + int(int_mode))
    tab = make_table(rng, int_mode, W, 64 * W - 37)
    protos, backfill = make_protos(rng, int_mode)
    proto_of = rng.integers(0, len(protos), size=n_tasks)
    cls = rng.integers(0, CLASSES, size=n_tasks)
    cls[: n_tasks // 2] = rng.integers(0, 2, size=n_tasks // 2)
    bits, F, FI = kr.scan_reference(tab, proto_of, protos, backfill, cls, 1, Wl, slots)
    # M at, below and above the number of fits, and 1. Never 0, and never exactly the fits of the
    # first 64 words with none after them: the select kernel stops before it has looked at the rest
    # and reports such a list as incomplete, which costs the host a rescan at most and which the
    # header's "fits remain" leaves open; no case here has such a row (the reference would differ).
    fits = kr.popcount(F[:, w_lo:w_hi]).sum(axis=1)
    M = np.array([max(1, (int(f), int(f) - 1, int(f) + 3, 1)[t % 4]) for t, f in enumerate(fits)])
    cap_off = np.concatenate([[0], np.cumsum(M)]).astype(np.uint32)
    p = dict(n_nodes=tab.n_nodes, W=W, Wl=Wl, slots=slots, tab_lo=0, stride=tab.stride, classes=CLASSES,
             n_tasks=n_tasks, cap_check=1, int_mode=1 if int_mode else 0, w_lo=w_lo, w_hi=w_hi)
    recs = kr.task_records(int_mode, protos, backfill, proto_of, cls)
    return dict(p=p, tab=tab, recs=recs, cap_off=cap_off, bits=bits, F=F, FI=FI, fits=fits, M=M)


# ---------------------------------------------------------------- FitError
def make_fit_case(seed, n_nodes, ends, window=None, cap_check=1, nq_extra=0):
    """A final table, a decision log over its nodes (some nodes without
    decisions, some with Pipelines only, some with Allocates after Pipelines)
    and an odd number of queries: consecutive ones (one workgroup) with
    different `end`, `point` before, between and after the decisions, the
    winner inside and outside the range."""
    rng = np.random.default_rng(seed)
    W = (n_nodes + 63) // 64
    tab = make_table(rng, False, W, n_nodes, window=window)
    _, pools = value_pools(False)
    D = n_nodes  # decisions in the log, first-fit style: piled on the low nodes
    node_of = np.minimum(rng.integers(0, n_nodes, size=D), rng.integers(0, n_nodes, size=D))
    pipeline = rng.random(D) < 0.4
    only_pipelines = rng.random(n_nodes) < 0.2
    pipeline |= only_pipelines[node_of]
    order = np.argsort(node_of, kind="stable")  # each node's decisions in log order
    hoff = np.concatenate([[0], np.cumsum(np.bincount(node_of, minlength=n_nodes))]).astype(np.int32)
    hk = (order.astype(np.uint32) | np.where(pipeline[order], 0x80000000, 0).astype(np.uint32)).view(np.int32)
    hold = np.stack([rng.choice(pools[d], size=D) for d in range(3)], axis=1).astype(np.float64)
    na = np.full(D, -1, dtype=np.int32)
    for n in range(n_nodes):  # the first Allocate at or after each decision on its node
        nxt = -1
        for e in range(int(hoff[n + 1]) - 1, int(hoff[n]) - 1, -1):
            if hk[e] >= 0:
                nxt = e
            na[e] = nxt
    tab.ntasks = (np.bincount(node_of, minlength=W * 64) + rng.integers(0, 3, size=W * 64)).astype(np.int32)
    tab.maxtasks = rng.integers(1, 6, size=W * 64).astype(np.int32)
    protos, _ = make_protos(rng, False)
    nq = len(ends) + nq_extra
    nq += 1 - nq % 2  # odd: the last workgroup holds one query
    q = np.zeros(nq, dtype=kr.FIT_QUERY)
    for i in range(nq):
        end = ends[i % len(ends)]
        q[i] = (int(rng.integers(0, 2)), end, (0, D // 3, D // 2, D, int(rng.integers(0, D + 1)))[i % 5],
                (-1, end // 2, end + 5, 0)[i % 4], protos[int(rng.integers(3, len(protos)))])
    p = dict(n_nodes=n_nodes, W=W, stride=tab.stride, classes=CLASSES, tab_lo=tab.tab_lo, tab_n=tab.tab_n, nq=nq,
             cap_check=cap_check, n_dec=D)
    return dict(p=p, tab=tab, hoff=hoff, hk=hk, hold=hold, na=na, q=q)


FIT_CASES = {
    "ends": dict(seed=8001, n_nodes=2100, ends=(1, 63, 64, 65, 1024, 1025, 2100)),
    "window": dict(seed=8002, n_nodes=2100, ends=(2100, 131, 1025, 64, 1700), window=(130, 1500)),
    "nocap": dict(seed=8003, n_nodes=1025, ends=(1025, 1024, 1), cap_check=0, nq_extra=4),
}


@functools.lru_cache(maxsize=None)
def fit_case(name):
    return make_fit_case(**FIT_CASES[name])
