// kbg_drain.ipp: where a node's running pods would land if it left.
// Part of kbg_session.cpp (one translation unit: included there inside its
// anonymous namespace, after kbg_node_why.ipp; not compiled on its own).

// ============================================================== node drain
// kbg_node_drain: each named node's movable tasks in NodeInfo.Tasks order,
// each to its first fitting node against a view private to the row in which
// the drained node and the cordon take nothing (kbg_device.hpp DrainArgs;
// allocate.go:105-171, backfill.go:47-64); nothing of the session changes.
// The host walk is host_job_fit (kbg_job_fit.ipp) with the exclusion test and
// the BestEffort branch.
// The session compiles predicate classes for its allocate and backfill
// candidates only, and a pod that runs on a node is neither. With the
// predicates plugin on, the call compiles the pod specs of the walked tasks
// into classes and stage planes of its own, as the session does for its
// candidates at open (compile_spec_classes, kbg_stage_mask_kernel), uses them
// for the walk and frees them. Host ports live in the session's candidate
// classes too (setup_host_ports): a walk that holds a pod with a host port is
// the host's, with the pod's own port entries against the node's used ports
// (DrainPorts, kbg_job_fit.ipp). Pod affinity is counted per candidate class
// (setup_affinity): in a session with pod affinity every walk is the host's,
// with the verdict of now per (walked spec, node) from the compiled terms and
// the AllocatedStatus pods themselves (aff_spec_verdicts, kbg_affinity.cpp).

// The call's own device blocks, given back when it returns.
struct DrainScratch {
  Session& S;
  std::vector<void*> blocks;
  explicit DrainScratch(Session& s) : S(s) {}
  void adopt(void* p) { blocks.push_back(p); }
  ~DrainScratch() {
    for (void* p : blocks) {
      auto it = std::find(S.d_allocs.begin(), S.d_allocs.end(), p);
      if (it == S.d_allocs.end()) continue;
      S.d_allocs.erase(it);
      pool_put(p);
    }
  }
};

kbg_status node_drain(Session& S, const int32_t* nodes, int32_t n_nodes, const int32_t* cordon, int32_t n_cordon,
                      int32_t limit, kbg_node_drain_row* out, kbg_fit_place* places, int32_t places_cap,
                      int32_t* n_places) {
  if (n_places) *n_places = 0;
  if (!S.opts.reasons) return fail(KBG_E_INVALID, "the session was opened without kbg_options.reasons");
  if (S.comm) return fail(KBG_E_UNSUPPORTED, "node drain on a session over a communicator");
  if (!S.stream) return fail(KBG_E_UNSUPPORTED, "node drain on a session without a device");
  if (n_nodes < 0 || (n_nodes > 0 && !out)) return fail(KBG_E_INVALID, "null argument");
  if (!nodes && n_nodes != S.n_nodes)
    return fail(KBG_E_INVALID, "nodes == NULL describes every node: n_nodes must be the node count");
  if (n_cordon < 0 || (n_cordon > 0 && !cordon)) return fail(KBG_E_INVALID, "cordon == NULL with a count");
  if (limit < 1 || limit > KBG_FIT_MAX_LIMIT) return fail(KBG_E_INVALID, "limit outside 1..512");
  if (places_cap < 0 || (!places && places_cap != 0)) return fail(KBG_E_INVALID, "places == NULL with a capacity");
  for (int32_t i = 0; nodes && i < n_nodes; ++i)
    if (nodes[i] < 0 || nodes[i] >= S.n_nodes) return fail(KBG_E_INVALID, "node index");
  for (int32_t i = 0; i < n_cordon; ++i)
    if (cordon[i] < 0 || cordon[i] >= S.n_nodes) return fail(KBG_E_INVALID, "cordon index");
  if (n_nodes == 0) return KBG_OK;
  if (kbg_status st = ensure_stage_planes(S); st != KBG_OK) return st;
  const kbg::StagePlanes hp0 = kbg::kbg_stage_planes(S.h_stage.data(), S.n_classes, S.W);
  auto live = [&](int32_t n) { return (bool)((hp0.live[n >> 6] >> (n & 63)) & 1ull); };
  // before the cycle's first action the session is its snapshot
  auto status = [&](int32_t t) { return S.cycle_started ? S.tstat[t] : (int32_t)S.tasks_in[t].status; };
  auto movable = [&](int32_t t) {  // AllocatedStatus, api/helpers.go:63-70
    if (!S.task_live[t]) return false;
    const int32_t st = status(t);
    return st == KBG_ALLOCATED || st == KBG_BINDING || st == KBG_BOUND || st == KBG_RUNNING;
  };

  // the cordon as a plane over the nodes (a dead node's bit changes nothing: `live` is and-ed in)
  std::vector<uint64_t> excl(S.W, 0);
  for (int32_t i = 0; i < n_cordon; ++i) excl[cordon[i] >> 6] |= 1ull << (cordon[i] & 63);

  // what the cycle's own actions put on each node so far, in the order of the decision log: an Allocate whose
  // task is still Allocated (Binding once its gang was dispatched) joins the node's tasks behind those it held at open, a Pipeline its other pods (a
  // decision that met its PodKey on the node left the node as it was, node_info.go:101-106)
  std::vector<std::vector<int32_t>> placed(S.cycle_started ? S.n_nodes : 0);
  std::vector<int32_t> piped(S.cycle_started ? S.n_nodes : 0, 0);
  if (S.cycle_started) {
    std::vector<char> once(S.n_tasks, 0);
    for (size_t k = 0; k < S.dec.size(); ++k) {
      const kbg_decision& d = S.dec[k];
      if (d.node < 0 || d.node >= S.n_nodes || (k < S.dec_dup.size() && S.dec_dup[k]) || once[d.task]) continue;
      if (d.kind == KBG_KIND_ALLOCATE && (S.tstat[d.task] == KBG_ALLOCATED || S.tstat[d.task] == KBG_BINDING)) {
        placed[d.node].push_back(d.task);
        once[d.task] = 1;
      } else if (d.kind == KBG_KIND_PIPELINE && S.tstat[d.task] == KBG_PIPELINED) {
        piped[d.node]++;
        once[d.task] = 1;
      }
    }
  }

  // the walks: per node its movable tasks in NodeInfo.Tasks order, the first `limit` of them
  std::vector<int32_t> walk, walk_off(n_nodes + 1, 0);
  for (int32_t i = 0; i < n_nodes; ++i) {
    const int32_t n = nodes ? nodes[i] : i;
    kbg_node_drain_row& o = out[i];
    o = kbg_node_drain_row{};
    walk_off[i + 1] = (int32_t)walk.size();
    if (!live(n)) continue;
    const size_t w0 = walk.size();
    int32_t tasks = 0;
    int32_t at_open = 0;  // of the movable tasks: those the node held at open
    for (const int32_t t : S.node_task_order[n])
      if (movable(t)) {
        if (tasks < limit) walk.push_back(t);
        ++tasks;
        ++at_open;
      }
    if (S.cycle_started)
      for (const int32_t t : placed[n]) {
        if (tasks < limit) walk.push_back(t);
        ++tasks;
      }
    walk_off[i + 1] = (int32_t)walk.size();
    o.valid = 1;
    o.node = n;
    o.tasks = tasks;
    o.walked = std::min(tasks, limit);
    o.first_unplaced = -1;
    o.other_pods = (int32_t)S.node_key_order[n].size() - at_open + (S.cycle_started ? piped[n] : 0);
    o.affinity_now = S.has_aff ? 1 : 0;
    o.place_off = places ? (int32_t)w0 : -1;
  }
  const int32_t total = (int32_t)walk.size();
  if (n_places) *n_places = total;
  if (places && total > places_cap)
    return fail(KBG_E_CAPACITY, "places buffer too small: need " + std::to_string(total));
  // the walked pods' own predicate classes and stage planes
  std::vector<int32_t> cls_of(total, 0);
  kbg::StagePlanes hp = hp0, dp = kbg::kbg_stage_planes(S.d_stage, S.n_classes, S.W);
  std::vector<uint64_t> h_own;
  DrainScratch scratch(S);
  DrainPorts dports;
  std::vector<std::vector<char>> aff_cls;  // [class][node] with pod affinity: the verdict of now
  bool any_port = false;  // a walked pod carries a host port: the host's
  if (S.pred_active && total > 0) {
    std::vector<int32_t> class_spec;
    std::unordered_map<int32_t, int32_t> class_of_spec;
    for (int32_t k = 0; k < total; ++k) {
      const int32_t sp = S.tasks_in[walk[k]].spec;
      auto [it, fresh] = class_of_spec.emplace(sp, (int32_t)class_spec.size());
      if (fresh) {
        class_spec.push_back(sp);
        dports.want.emplace_back();
        for (int32_t i = 0; sp >= 0 && i < S.specs_in[sp].port_len; ++i) {
          const kbg_host_port& hp = S.ports_in[S.specs_in[sp].port_off + i];
          if (hp.host_port <= 0) continue;
          dports.want.back().push_back(raw_port(S, hp));
          any_port = true;
        }
      }
      cls_of[k] = it->second;
    }
    if (any_port && S.has_ports) {  // the atoms each class conflicts with (the dictionary holds every used port)
      dports.conf.assign(class_spec.size() * (size_t)S.PW, 0);
      for (const auto& kv : S.atom_of) {
        const size_t p1 = kv.first.find('|'), p2 = kv.first.rfind('|');
        const RawPort used{kv.first.substr(0, p1), kv.first.substr(p1 + 1, p2 - p1 - 1), atoi(kv.first.c_str() + p2 + 1)};
        for (size_t c = 0; c < class_spec.size(); ++c)
          for (const RawPort& a : dports.want[c])
            if (port_conflict(a, used)) dports.conf[c * S.PW + kv.second / 64] |= 1ull << (kv.second % 64);
      }
    }
    if (S.has_aff) {
      // pod affinity as it is now, for every step: the AllocatedStatus pods of now, each on its node (the moved
      // pods still count where they are), against the terms of each walked spec
      std::vector<std::pair<int32_t, int32_t>> pods;
      std::vector<int32_t> node_now(S.n_tasks, -2);
      for (int32_t n = 0; S.cycle_started && n < S.n_nodes; ++n)
        for (const int32_t t : placed[n]) node_now[t] = n;
      for (int32_t t = 0; t < S.n_tasks; ++t)
        if (movable(t)) pods.emplace_back(S.tasks_in[t].spec, node_now[t] != -2 ? node_now[t] : S.task_node[t]);
      aff_cls.resize(class_spec.size());
      for (size_t c = 0; c < class_spec.size(); ++c) kbg::aff_spec_verdicts(S, class_spec[c], pods, &aff_cls[c]);
    }
    kbg::StaticHost sh;
    kbg::compile_spec_classes(S, class_spec, &sh);
    if (S.node_flags.size() == sh.node_flags.size()) sh.node_flags = S.node_flags;  // dead nodes as the session has them
    kbg::StaticTables t{};
    uint64_t *lb, *tb, *mp, *tp;
    int64_t* nv;
    uint8_t *nok, *nf;
    int32_t* nid;
    kbg::ReqProg* rq;
    kbg::TermProg* tm;
    kbg::ClassProg* cl;
    BulkUpload bu;
    bu.add(&lb, sh.label_bits);
    bu.add(&tb, sh.taint_bits);
    bu.add(&mp, sh.mask_pool);
    bu.add(&tp, sh.tol_pool);
    bu.add(&nv, sh.num_vals);
    bu.add(&nok, sh.num_ok);
    bu.add(&nf, sh.node_flags);
    bu.add(&nid, sh.name_id);
    bu.add(&rq, sh.reqs);
    bu.add(&tm, sh.terms);
    bu.add(&cl, sh.classes);
    if (kbg_status st = bu.commit(S); st != KBG_OK) return st;
    scratch.adopt(lb);  // (the block's first item: its base)
    t.n_nodes = S.n_nodes, t.label_words = sh.label_words, t.taint_words = sh.taint_words, t.n_numcols = sh.n_numcols;
    t.label_bits = lb, t.taint_bits = tb, t.num_vals = nv, t.num_ok = nok, t.name_id = nid, t.node_flags = nf;
    t.mask_pool = mp, t.tol_pool = tp, t.reqs = rq, t.terms = tm, t.classes = cl;
    const size_t words = kbg::kbg_stage_words(sh.n_classes, S.W);
    uint64_t* d_own = nullptr;
    if (kbg_status st = dalloc(S, &d_own, words); st != KBG_OK) return st;
    scratch.adopt(d_own);
    dp = kbg::kbg_stage_planes(d_own, sh.n_classes, S.W);
    HIP_TRY(kbg::launch_build_stage_planes(t, sh.n_classes, S.W, dp, S.stream));
    h_own.resize(words);
    HIP_TRY(hipMemcpyAsync(h_own.data(), d_own, words * 8, hipMemcpyDeviceToHost, S.stream));
    HIP_TRY(hipStreamSynchronize(S.stream));
    hp = kbg::kbg_stage_planes(h_own.data(), sh.n_classes, S.W);
  }
  std::vector<kbg_fit_place> own;
  if (!places) {
    own.resize(std::max(total, 1));
    places = own.data();
  }
  int32_t panic_nodes = 0;
  for (int32_t n = 0; n < S.n_nodes; ++n)
    if (live(n) && S.panic_node[n]) ++panic_nodes;

  // The device knows the static stages, Idle, Releasing and the pod counts; a
  // nil Node and a PodKey that can meet itself on a node are the host's, as is
  // a table past the kernel's bitmap (host ports and pod affinity: see above).
  // KBG_HOST_NODE_DRAIN, read per call, asks for the host on any session (A/B
  // parity tests, as KBG_HOST_JOB_FIT).
  const char* env = getenv("KBG_HOST_NODE_DRAIN");
  const bool host_only = any_port || S.has_aff || S.any_nil || S.has_dupkeys || S.tab_n > kbg::kFitMaxNodes ||
                         (env && env[0] == '1');
  if (total == 0) {
    // nothing to walk: the rows are complete but for panic_nodes
  } else if (host_only) {
    for (int32_t i = 0; i < n_nodes; ++i) {
      if (walk_off[i] == walk_off[i + 1]) continue;
      const std::vector<int32_t> w(walk.begin() + walk_off[i], walk.begin() + walk_off[i + 1]);
      host_job_fit(S, hp, nullptr, w, places + walk_off[i], excl.data(), out[i].node, cls_of.data() + walk_off[i],
                   any_port ? &dports : nullptr, S.has_aff ? &aff_cls : nullptr);
    }
  } else {
    kbg_status st;
    // node rows and mask words a victim action staged but has not pushed yet
    if (S.vt_ready && (!S.sdeltas.empty() || !S.mask_dirty.empty()))
      if ((st = victim_push(S, std::vector<int32_t>{})) != KBG_OK) return st;
    // the launch's distinct shapes by (class, BestEffort, request bits), and per walk the cursor links
    std::vector<kbg::TaskShape> shapes;
    std::vector<char> cursor;  // the shape has no negative request dimension
    std::map<std::tuple<int32_t, uint64_t, uint64_t, uint64_t>, int32_t> seen;  // (IsEmpty() follows from the request)
    auto bits = [](double v) {
      uint64_t u;
      std::memcpy(&u, &v, 8);
      return u;
    };
    std::vector<kbg::JobFitStep> steps(total);
    std::vector<int32_t> last, last_walk;  // per shape: its last step in the current walk, as (walk stamp, index)
    std::vector<int32_t> rows(n_nodes, -1);
    for (int32_t i = 0; i < n_nodes; ++i) {
      if (out[i].valid) rows[i] = out[i].node - S.tab_lo;  // (outside [0, tab_n): excludes nothing)
      if (rows[i] < -1) rows[i] = -1;
      for (int32_t k = walk_off[i]; k < walk_off[i + 1]; ++k) {
        const int32_t t = walk[k];
        const Res& r = S.treq[t];
        auto [it, fresh] = seen.emplace(std::make_tuple(cls_of[k], bits(r.c), bits(r.m), bits(r.g)),
                                        (int32_t)shapes.size());
        if (fresh) {
          shapes.push_back(
              kbg::TaskShape{cls_of[k], kbg::res_empty(r) ? kbg::kTaskShapeBestEffort : 0, {r.c, r.m, r.g}});
          cursor.push_back(!(r.c < 0 || r.m < 0 || r.g < 0));
          last.push_back(-1);
          last_walk.push_back(-1);
        }
        const int32_t s = it->second;
        steps[k].shape = s;
        steps[k].prev = cursor[s] && last_walk[s] == i ? last[s] : -1;
        last[s] = k - walk_off[i];
        last_walk[s] = i;
      }
    }
    const int32_t Q = (int32_t)shapes.size();
    constexpr int32_t kChunk = 4096;  // walks per launch
    size_t step_cap = 0;              // the most steps a chunk holds
    for (int32_t j0 = 0; j0 < n_nodes; j0 += kChunk)
      step_cap = std::max<size_t>(step_cap, walk_off[std::min(n_nodes, j0 + kChunk)] - walk_off[j0]);
    const size_t walk_cap = (size_t)std::min(n_nodes, kChunk) + 1;
    if (S.drain_shape_cap < (size_t)Q || S.drain_step_cap < step_cap || S.drain_walk_cap < walk_cap ||
        S.drain_excl_cap < (size_t)S.W) {
      for (void* p : {(void*)S.d_drain_shapes, (void*)S.d_drain_steps, (void*)S.d_drain_off, (void*)S.d_drain_row,
                      (void*)S.d_drain_out, (void*)S.d_drain_excl})
        if (p) {
          pool_put(p);
          S.d_allocs.erase(std::find(S.d_allocs.begin(), S.d_allocs.end(), p));
        }
      S.d_drain_shapes = nullptr;
      S.d_drain_steps = nullptr;
      S.d_drain_off = S.d_drain_row = S.d_drain_out = nullptr;
      S.d_drain_excl = nullptr;
      const size_t qc = std::max(S.drain_shape_cap, (size_t)Q), sc = std::max(S.drain_step_cap, step_cap);
      const size_t wc = std::max(S.drain_walk_cap, walk_cap), xc = std::max(S.drain_excl_cap, (size_t)S.W);
      S.drain_shape_cap = S.drain_step_cap = S.drain_walk_cap = S.drain_excl_cap = 0;
      if ((st = dalloc(S, &S.d_drain_shapes, qc)) != KBG_OK) return st;
      if ((st = dalloc(S, &S.d_drain_steps, sc)) != KBG_OK) return st;
      if ((st = dalloc(S, &S.d_drain_off, wc)) != KBG_OK) return st;
      if ((st = dalloc(S, &S.d_drain_row, wc)) != KBG_OK) return st;
      if ((st = dalloc(S, &S.d_drain_out, sc * 2)) != KBG_OK) return st;
      if ((st = dalloc(S, &S.d_drain_excl, xc)) != KBG_OK) return st;
      S.drain_shape_cap = qc, S.drain_step_cap = sc, S.drain_walk_cap = wc, S.drain_excl_cap = xc;
    }
    HIP_TRY(hipMemcpyAsync(S.d_drain_shapes, shapes.data(), (size_t)Q * sizeof(kbg::TaskShape), hipMemcpyHostToDevice,
                           S.stream));
    HIP_TRY(hipMemcpyAsync(S.d_drain_excl, excl.data(), (size_t)S.W * sizeof(uint64_t), hipMemcpyHostToDevice,
                           S.stream));
    std::vector<int32_t> off, res;
    double drain_ms = 0;  // event time of the kbg_drain_kernel launches
    int32_t launches = 0;
    for (int32_t j0 = 0; j0 < n_nodes; j0 += kChunk) {
      const int32_t nj = std::min(kChunk, n_nodes - j0), k0 = walk_off[j0], nk = walk_off[j0 + nj] - k0;
      if (nk == 0) continue;
      off.resize(nj + 1);
      for (int32_t i = 0; i <= nj; ++i) off[i] = walk_off[j0 + i] - k0;
      res.resize((size_t)nk * 2);
      HIP_TRY(hipMemcpyAsync(S.d_drain_steps, steps.data() + k0, (size_t)nk * sizeof(kbg::JobFitStep),
                             hipMemcpyHostToDevice, S.stream));
      HIP_TRY(hipMemcpyAsync(S.d_drain_off, off.data(), (size_t)(nj + 1) * sizeof(int32_t), hipMemcpyHostToDevice,
                             S.stream));
      HIP_TRY(hipMemcpyAsync(S.d_drain_row, rows.data() + j0, (size_t)nj * sizeof(int32_t), hipMemcpyHostToDevice,
                             S.stream));
      kbg::DrainArgs a{};
      a.nodes = S.d_nodes.idle_cpu, a.stride = soa_stride(S), a.W = S.W, a.tab_lo = S.tab_lo, a.tab_n = S.tab_n;
      a.sel_ok = dp.sel_ok, a.taint_ok = dp.taint_ok, a.unsched = dp.unsched, a.live = dp.live;
      a.excl = S.d_drain_excl;
      a.shapes = S.d_drain_shapes, a.steps = S.d_drain_steps, a.walk_off = S.d_drain_off, a.walk_row = S.d_drain_row;
      a.n_shapes = Q, a.n_walks = nj, a.cap_check = S.pred_active ? 1 : 0;
      a.out = S.d_drain_out;
      a.h_shapes = shapes.data(), a.h_steps = steps.data() + k0, a.h_walk_off = off.data();
      a.h_walk_row = rows.data() + j0;
      HIP_TRY(kbg::launch_drain(a, S.stream, S.ev[0], S.ev[1]));
      HIP_TRY(hipMemcpyAsync(res.data(), S.d_drain_out, (size_t)nk * 2 * sizeof(int32_t), hipMemcpyDeviceToHost,
                             S.stream));
      HIP_TRY(hipStreamSynchronize(S.stream));  // (the staging vectors are rewritten by the next chunk)
      if (S.tab_n > 0) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
        drain_ms += ms;
        ++launches;
      }
      for (int32_t k = 0; k < nk; ++k)
        places[k0 + k] = kbg_fit_place{walk[k0 + k], S.tab_n > 0 ? res[2 * k] : -1, S.tab_n > 0 ? res[2 * k + 1] : 0, 0};
    }
    S.vstage_busy = false;
    if (getenv("KBG_PROFILE_NODE_DRAIN"))
      fprintf(stderr, "[kbg node drain] %d walks, %d steps, %d shapes, limit %d, %d launches, drain kernel %.3f ms\n",
              n_nodes, total, Q, limit, launches, drain_ms);
  }
  // the rows, from the places
  std::vector<int32_t> used, lost_job;  // per row: the nodes taking a task; the job of each unplaced task
  for (int32_t i = 0; i < n_nodes; ++i) {
    kbg_node_drain_row& o = out[i];
    if (!o.valid) continue;
    o.panic_nodes = panic_nodes;
    used.clear();
    lost_job.clear();
    std::vector<int32_t> jobs;
    for (int32_t k = walk_off[i]; k < walk_off[i + 1]; ++k) {
      const kbg_fit_place& p = places[k];
      jobs.push_back(S.task_job[p.task]);
      if (p.node < 0) {
        if (o.first_unplaced < 0) o.first_unplaced = p.task;
        o.unplaced++;
        lost_job.push_back(S.task_job[p.task]);
        continue;
      }
      (p.kind == KBG_KIND_ALLOCATE ? o.placed_idle : o.placed_releasing)++;
      used.push_back(p.node);
    }
    std::sort(used.begin(), used.end());
    o.nodes_used = (int32_t)(std::unique(used.begin(), used.end()) - used.begin());
    std::sort(jobs.begin(), jobs.end());
    o.jobs_moved = (int32_t)(std::unique(jobs.begin(), jobs.end()) - jobs.begin());
    // a gang that is ready now and is not without its unplaced tasks (gang.go:44-78)
    std::sort(lost_job.begin(), lost_job.end());
    for (size_t a = 0; a < lost_job.size();) {
      size_t b = a;
      while (b < lost_job.size() && lost_job[b] == lost_job[a]) ++b;
      const int32_t j = lost_job[a], ready = S.cycle_started ? S.committed_ready[j] : S.job_ready0[j];
      const int32_t need = S.jobs_in[j].min_available;
      if (ready >= need && ready - (int32_t)(b - a) < need) o.jobs_short++;
      a = b;
    }
  }
  return KBG_OK;
}
