// kbg_job_fit.ipp: where a job's Pending tasks would land now.
// Part of kbg_session.cpp (one translation unit: included there inside its
// anonymous namespace, after kbg_headroom.ipp; not compiled on its own).

// ================================================================= job fit
// kbg_job_fit: each named job's Pending tasks with a request, in TaskOrderFn
// order, each to its first fitting node against a view private to the job in
// which every placement takes what the next task no longer sees
// (kbg_device.hpp JobFitArgs; allocate.go:105-171); nothing of the session
// changes.

// The walk of one job on the host mirror, the definition of the device walk
// with what the device does not know: host ports through the view (the pod's
// ports join the node's, predicates.go:143-155), the PodKey a node already
// holds (node_info.go:101-106: the placement is reported, the view stays), pod
// affinity as it is now, nil Nodes. `view` maps a touched node to its state.
// The cursor is the device's (kbg_device.hpp JobFitArgs): a (class, request)
// starts at the node its previous step landed on, or lands nowhere where that
// step did; ports, keys and pods only join the view, so a node that turned
// the shape away keeps turning it away here too.
struct FitView {
  Res idle, rel;
  int32_t nt;
  std::vector<uint64_t> ports;  // [PW] with host ports
  std::vector<int32_t> joined;  // kbg_node_drain: the caller's classes with host ports the walk placed here
};
// The host ports of kbg_node_drain's own classes (kbg_drain.ipp): per class the
// wanted (ip, protocol, port) entries as host_ports.go compares them, and, in a
// session that keeps port atoms, the atoms each class conflicts with.
struct RawPort {
  std::string ip, proto;
  int32_t port;
};
inline bool port_conflict(const RawPort& a, const RawPort& b) {  // host_ports.go CheckConflict
  return a.proto == b.proto && a.port == b.port && (a.ip == "0.0.0.0" || b.ip == "0.0.0.0" || a.ip == b.ip);
}
struct DrainPorts {
  std::vector<std::vector<RawPort>> want;  // [class]
  std::vector<uint64_t> conf;              // [class][PW], with S.has_ports
};
inline RawPort raw_port(const Session& S, const kbg_host_port& hp) {
  return RawPort{S.strs[hp.host_ip].empty() ? std::string("0.0.0.0") : S.strs[hp.host_ip],
                 S.strs[hp.protocol].empty() ? std::string("TCP") : S.strs[hp.protocol], hp.host_port};
}
// kbg_node_drain's walk is this one with two more rules (kbg_drain.ipp):
// `excl` (a plane over the nodes, or null) and `xnode` (or -1) take nothing,
// with the predicates plugin off as well, and a task with an empty request
// goes to the first node past the stages with no resource test
// (backfill.go:47-64). kbg_job_fit passes neither and walks no such task.
// `cls_of` gives each step a class of the caller's own planes `sp` in place of
// the session's, and `dports` those classes' host ports: a node's used ports
// are the session's atoms of now (or, in a session that keeps none, the
// entries of its pods at open: no candidate wants a port, so no action changes
// them), and the ports of the walk's own placements join them in the view
// (predicates.go:143-155). `aff_cls` holds those classes' pod affinity verdicts
// of now per node, applied to every step.
void host_job_fit(Session& S, const kbg::StagePlanes& sp, const kbg::AffState* aff, const std::vector<int32_t>& walk,
                  kbg_fit_place* places, const uint64_t* excl = nullptr, int32_t xnode = -1,
                  const int32_t* cls_of = nullptr, const DrainPorts* dports = nullptr,
                  const std::vector<std::vector<char>>* aff_cls = nullptr) {
  const bool ports = S.has_ports && !cls_of, affinity = S.has_aff && !cls_of;
  std::unordered_map<int32_t, FitView> view;
  std::unordered_set<int64_t> keys;  // (node << 32 | key) the walk added
  std::map<std::tuple<int32_t, uint64_t, uint64_t, uint64_t>, int32_t> cursor;  // n_nodes: nowhere
  auto bits = [](double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return u;
  };
  for (size_t i = 0; i < walk.size(); ++i) {
    const int32_t t = walk[i], cls = cls_of ? cls_of[i] : S.task_class[t];
    const Res& q = S.treq[t];
    int32_t* from = q.c < 0 || q.m < 0 || q.g < 0 ? nullptr : &cursor[std::make_tuple(cls, bits(q.c), bits(q.m), bits(q.g))];
    const bool hot = S.has_dupkeys && S.key_hot[S.task_key[t]];
    const bool beff = kbg::res_empty(q);
    kbg_fit_place& o = places[i];
    o = kbg_fit_place{t, -1, KBG_KIND_ALLOCATE, 0};
    for (int32_t n = from ? *from : 0; n < S.n_nodes; ++n) {
      const uint64_t bit = 1ull << (n & 63);
      if (!(sp.live[n >> 6] & bit)) continue;
      if (n == xnode || (excl && (excl[n >> 6] & bit))) continue;
      if (S.panic_node[n]) continue;  // predicates.go:122-123
      const auto it = view.find(n);
      const FitView* v = it == view.end() ? nullptr : &it->second;
      if (S.pred_active) {
        const size_t w = (size_t)cls * S.W + (n >> 6);
        if ((v ? v->nt : S.ntasks[n]) >= S.maxtasks[n]) continue;
        if (!(sp.sel_ok[w] & bit)) continue;
        if (ports) {
          const uint64_t* np = v ? v->ports.data() : &S.node_ports[(size_t)n * S.PW];
          bool conflict = false;
          for (int32_t pw = 0; pw < S.PW; ++pw) conflict = conflict || (np[pw] & S.cls_conf[(size_t)cls * S.PW + pw]);
          if (conflict) continue;
        }
        if (dports && !dports->want[cls].empty()) {
          const std::vector<RawPort>& want = dports->want[cls];
          bool conflict = false;
          if (S.has_ports) {
            for (int32_t pw = 0; pw < S.PW; ++pw)
              conflict = conflict || (S.node_ports[(size_t)n * S.PW + pw] & dports->conf[(size_t)cls * S.PW + pw]);
          } else {
            const kbg_node& nd = S.nodes_in[n];
            for (int32_t k = 0; k < nd.port_len && !conflict; ++k) {
              const kbg_host_port& hp = S.ports_in[nd.port_off + k];
              if (hp.host_port <= 0) continue;
              const RawPort used = raw_port(S, hp);
              for (const RawPort& a : want) conflict = conflict || port_conflict(a, used);
            }
          }
          for (size_t k = 0; v && k < v->joined.size() && !conflict; ++k)
            for (const RawPort& b : dports->want[v->joined[k]])
              for (const RawPort& a : want) conflict = conflict || port_conflict(a, b);
          if (conflict) continue;
        }
        if (sp.unsched[n >> 6] & bit) continue;
        if (!(sp.taint_ok[w] & bit)) continue;
        if (affinity && !kbg::aff_ok(S, *aff, cls, n)) continue;
        if (aff_cls && !(*aff_cls)[cls][n]) continue;  // the caller's classes: today's verdict (predicates.go:185-198)
      }
      int32_t kind;
      if (beff) kind = KBG_KIND_ALLOCATE;  // backfill.go:47-64: no resource test
      else if (kbg::res_le(q, v ? v->idle : S.idle[n])) kind = KBG_KIND_ALLOCATE;  // allocate.go:136-146
      else if (kbg::res_le(q, v ? v->rel : S.rel[n])) kind = KBG_KIND_PIPELINE;  // allocate.go:148-162
      else continue;
      o.node = n;
      o.kind = kind;
      const int64_t nk = node_key_of(S, t, n);
      if (hot && (S.node_keys.count(nk) || keys.count(nk))) break;  // AddTask's error: the node is unchanged
      FitView& u = view[n];
      if (!v) {
        u.idle = S.idle[n], u.rel = S.rel[n], u.nt = S.ntasks[n];
        if (ports) u.ports.assign(&S.node_ports[(size_t)n * S.PW], &S.node_ports[(size_t)n * S.PW] + S.PW);
      }
      if (!S.nil_node[n]) {
        Res& x = kind == KBG_KIND_ALLOCATE ? u.idle : u.rel;
        x.c -= q.c, x.m -= q.m, x.g -= q.g;  // Resource.Sub, plain fp64 (resource_info.go:100-110)
      }
      u.nt++;
      if (ports)
        for (int32_t pw = 0; pw < S.PW; ++pw) u.ports[pw] |= S.cls_add[(size_t)cls * S.PW + pw];
      if (dports && !dports->want[cls].empty()) u.joined.push_back(cls);
      if (hot) keys.insert(nk);
      break;
    }
    if (from) *from = o.node < 0 ? S.n_nodes : o.node;
  }
}

kbg_status job_fit(Session& S, const int32_t* jobs, int32_t n_jobs, int32_t limit, kbg_job_fit_row* out,
                   kbg_fit_place* places, int32_t places_cap, int32_t* n_places) {
  if (n_places) *n_places = 0;
  if (!S.opts.reasons) return fail(KBG_E_INVALID, "the session was opened without kbg_options.reasons");
  if (S.comm) return fail(KBG_E_UNSUPPORTED, "job fit on a session over a communicator");
  if (!S.stream) return fail(KBG_E_UNSUPPORTED, "job fit on a session without a device");
  if (n_jobs < 0 || (n_jobs > 0 && !out)) return fail(KBG_E_INVALID, "null argument");
  if (!jobs && n_jobs != S.n_jobs)
    return fail(KBG_E_INVALID, "jobs == NULL describes every job: n_jobs must be the job count");
  if (limit < 1 || limit > KBG_FIT_MAX_LIMIT) return fail(KBG_E_INVALID, "limit outside 1..512");
  if (places_cap < 0 || (!places && places_cap != 0)) return fail(KBG_E_INVALID, "places == NULL with a capacity");
  for (int32_t i = 0; jobs && i < n_jobs; ++i)
    if (jobs[i] < 0 || jobs[i] >= S.n_jobs) return fail(KBG_E_INVALID, "job index");
  if (n_jobs == 0) return KBG_OK;
  // before the cycle's first action the session is its snapshot
  const Engine& E = S.cycle_started ? S.fin : S.init;
  auto status = [&](int32_t t) { return S.cycle_started ? S.tstat[t] : (int32_t)S.tasks_in[t].status; };

  // the walks: per job its Pending tasks with a request in TaskOrderFn order
  // (pending_by_job's strict order), the first `limit` of them
  std::vector<int32_t> walk, walk_off(n_jobs + 1, 0);
  for (int32_t i = 0; i < n_jobs; ++i) {
    const int32_t j = jobs ? jobs[i] : i;
    kbg_job_fit_row& o = out[i];
    o = kbg_job_fit_row{};
    const size_t w0 = walk.size();
    for (int32_t k = S.jt_off[j]; k < S.jt_off[j + 1]; ++k) {
      const int32_t t = S.jt[k];
      if (S.task_live[t] && status(t) == KBG_PENDING && !kbg::res_empty(S.treq[t])) walk.push_back(t);
    }
    std::sort(walk.begin() + w0, walk.end(), [&](int32_t a, int32_t c) {
      if (S.task_order_prio && S.tasks_in[a].priority != S.tasks_in[c].priority)
        return S.tasks_in[a].priority > S.tasks_in[c].priority;
      return S.task_rank[a] < S.task_rank[c];
    });
    const int32_t pending = (int32_t)(walk.size() - w0);
    walk.resize(w0 + std::min(pending, limit));
    walk_off[i + 1] = (int32_t)walk.size();
    if (pending == 0) continue;
    o.valid = 1;
    o.job = j;
    o.pending = pending;
    o.walked = std::min(pending, limit);
    o.first_unplaced = -1;
    o.ready_num = S.cycle_started ? S.committed_ready[j] : S.job_ready0[j];
    o.min_available = S.jobs_in[j].min_available;
    const int32_t q = S.job_queue[j];
    o.queue_overused = S.has_prop && S.q_has_attr[q] && kbg::res_le(S.q_deserved[q], E.qalloc[q]) ? 1 : 0;
    o.affinity_now = S.has_aff ? 1 : 0;
    o.place_off = places ? (int32_t)w0 : -1;
  }
  const int32_t total = (int32_t)walk.size();
  if (n_places) *n_places = total;
  if (places && total > places_cap)
    return fail(KBG_E_CAPACITY, "places buffer too small: need " + std::to_string(total));
  if (total == 0) return KBG_OK;
  if (kbg_status st = ensure_stage_planes(S); st != KBG_OK) return st;
  const kbg::StagePlanes hp = kbg::kbg_stage_planes(S.h_stage.data(), S.n_classes, S.W);
  std::vector<kbg_fit_place> own;
  if (!places) {
    own.resize(total);
    places = own.data();
  }
  int32_t panic_nodes = 0;
  for (int32_t n = 0; n < S.n_nodes; ++n)
    if (((hp.live[n >> 6] >> (n & 63)) & 1ull) && S.panic_node[n]) ++panic_nodes;

  // The device knows the static stages, Idle, Releasing and the pod counts;
  // host ports, pod affinity, a nil Node and a PodKey that can meet itself on a
  // node are the host's, as is a table past the kernel's bitmap.
  // KBG_HOST_JOB_FIT, read per call, asks for the host on any session (A/B
  // parity tests, as KBG_HOST_TASK_HEADROOM).
  const char* env = getenv("KBG_HOST_JOB_FIT");
  const bool host_only = S.has_ports || S.has_aff || S.any_nil || S.has_dupkeys || S.tab_n > kbg::kFitMaxNodes ||
                         (env && env[0] == '1');
  if (host_only) {
    const kbg::AffState* aff = S.has_aff ? (S.cycle_started ? &S.affm->st : &S.affm->st0) : nullptr;
    for (int32_t i = 0; i < n_jobs; ++i) {
      const std::vector<int32_t> w(walk.begin() + walk_off[i], walk.begin() + walk_off[i + 1]);
      host_job_fit(S, hp, aff, w, places + walk_off[i]);
    }
  } else {
    kbg_status st;
    // node rows and mask words a victim action staged but has not pushed yet
    if (S.vt_ready && (!S.sdeltas.empty() || !S.mask_dirty.empty()))
      if ((st = victim_push(S, std::vector<int32_t>{})) != KBG_OK) return st;
    // the launch's distinct shapes by (class, request bits), and per job the cursor links
    std::vector<kbg::TaskShape> shapes;
    std::vector<char> cursor;  // the shape has no negative request dimension
    std::map<std::tuple<int32_t, uint64_t, uint64_t, uint64_t>, int32_t> seen;
    auto bits = [](double v) {
      uint64_t u;
      std::memcpy(&u, &v, 8);
      return u;
    };
    std::vector<kbg::JobFitStep> steps(total);
    std::vector<int32_t> last;  // per shape: its last step in the current job, as (job stamp, index)
    std::vector<int32_t> last_job;
    for (int32_t i = 0; i < n_jobs; ++i)
      for (int32_t k = walk_off[i]; k < walk_off[i + 1]; ++k) {
        const int32_t t = walk[k];
        const Res& r = S.treq[t];
        auto [it, fresh] = seen.emplace(std::make_tuple(S.task_class[t], bits(r.c), bits(r.m), bits(r.g)),
                                        (int32_t)shapes.size());
        if (fresh) {
          shapes.push_back(kbg::TaskShape{S.task_class[t], 0, {r.c, r.m, r.g}});
          cursor.push_back(!(r.c < 0 || r.m < 0 || r.g < 0));
          last.push_back(-1);
          last_job.push_back(-1);
        }
        const int32_t s = it->second;
        steps[k].shape = s;
        steps[k].prev = cursor[s] && last_job[s] == i ? last[s] : -1;
        last[s] = k - walk_off[i];
        last_job[s] = i;
      }
    const int32_t Q = (int32_t)shapes.size();
    constexpr int32_t kChunk = 4096;  // jobs per launch
    size_t step_cap = 0;              // the most steps a chunk holds
    for (int32_t j0 = 0; j0 < n_jobs; j0 += kChunk)
      step_cap = std::max<size_t>(step_cap, walk_off[std::min(n_jobs, j0 + kChunk)] - walk_off[j0]);
    const size_t job_cap = (size_t)std::min(n_jobs, kChunk) + 1;
    if (S.fit_shape_cap < (size_t)Q || S.fit_step_cap < step_cap || S.fit_job_cap < job_cap) {
      for (void* p : {(void*)S.d_fit_shapes, (void*)S.d_fit_steps, (void*)S.d_fit_off, (void*)S.d_fit_out})
        if (p) {
          pool_put(p);
          S.d_allocs.erase(std::find(S.d_allocs.begin(), S.d_allocs.end(), p));
        }
      S.d_fit_shapes = nullptr;
      S.d_fit_steps = nullptr;
      S.d_fit_off = nullptr;
      S.d_fit_out = nullptr;
      S.fit_shape_cap = S.fit_step_cap = S.fit_job_cap = 0;
      const size_t qc = std::max(S.fit_shape_cap, (size_t)Q), sc = std::max(S.fit_step_cap, step_cap);
      if ((st = dalloc(S, &S.d_fit_shapes, qc)) != KBG_OK) return st;
      if ((st = dalloc(S, &S.d_fit_steps, sc)) != KBG_OK) return st;
      if ((st = dalloc(S, &S.d_fit_off, job_cap)) != KBG_OK) return st;
      if ((st = dalloc(S, &S.d_fit_out, sc * 2)) != KBG_OK) return st;
      S.fit_shape_cap = qc, S.fit_step_cap = sc, S.fit_job_cap = job_cap;
    }
    const kbg::StagePlanes dp = kbg::kbg_stage_planes(S.d_stage, S.n_classes, S.W);
    HIP_TRY(hipMemcpyAsync(S.d_fit_shapes, shapes.data(), (size_t)Q * sizeof(kbg::TaskShape), hipMemcpyHostToDevice,
                           S.stream));
    std::vector<int32_t> off, res;
    double fit_ms = 0;  // event time of the kbg_job_fit_kernel launches
    for (int32_t j0 = 0; j0 < n_jobs; j0 += kChunk) {
      const int32_t nj = std::min(kChunk, n_jobs - j0), k0 = walk_off[j0], nk = walk_off[j0 + nj] - k0;
      if (nk == 0) continue;
      off.resize(nj + 1);
      for (int32_t i = 0; i <= nj; ++i) off[i] = walk_off[j0 + i] - k0;
      res.resize((size_t)nk * 2);
      HIP_TRY(hipMemcpyAsync(S.d_fit_steps, steps.data() + k0, (size_t)nk * sizeof(kbg::JobFitStep),
                             hipMemcpyHostToDevice, S.stream));
      HIP_TRY(hipMemcpyAsync(S.d_fit_off, off.data(), (size_t)(nj + 1) * sizeof(int32_t), hipMemcpyHostToDevice,
                             S.stream));
      kbg::JobFitArgs a{};
      a.nodes = S.d_nodes.idle_cpu, a.stride = soa_stride(S), a.W = S.W, a.tab_lo = S.tab_lo, a.tab_n = S.tab_n;
      a.sel_ok = dp.sel_ok, a.taint_ok = dp.taint_ok, a.unsched = dp.unsched, a.live = dp.live;
      a.shapes = S.d_fit_shapes, a.steps = S.d_fit_steps, a.job_off = S.d_fit_off;
      a.n_shapes = Q, a.n_jobs = nj, a.cap_check = S.pred_active ? 1 : 0;
      a.out = S.d_fit_out;
      a.h_shapes = shapes.data(), a.h_steps = steps.data() + k0, a.h_job_off = off.data();
      HIP_TRY(kbg::launch_job_fit(a, S.stream, S.ev[0], S.ev[1]));
      HIP_TRY(hipMemcpyAsync(res.data(), S.d_fit_out, (size_t)nk * 2 * sizeof(int32_t), hipMemcpyDeviceToHost,
                             S.stream));
      HIP_TRY(hipStreamSynchronize(S.stream));  // (the staging vectors are rewritten by the next chunk)
      if (S.tab_n > 0) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
        fit_ms += ms;
      }
      for (int32_t k = 0; k < nk; ++k)
        places[k0 + k] = kbg_fit_place{walk[k0 + k], S.tab_n > 0 ? res[2 * k] : -1, S.tab_n > 0 ? res[2 * k + 1] : 0, 0};
    }
    S.vstage_busy = false;
    if (getenv("KBG_PROFILE_JOB_FIT"))
      fprintf(stderr, "[kbg job fit] %d jobs, %d steps, %d shapes, limit %d, fit kernel %.3f ms\n", n_jobs, total, Q,
              limit, fit_ms);
  }
  // the rows, from the places
  for (int32_t i = 0; i < n_jobs; ++i) {
    kbg_job_fit_row& o = out[i];
    if (!o.valid) continue;
    o.panic_nodes = panic_nodes;
    o.ready_after = o.ready_num >= o.min_available ? 0 : -1;
    std::vector<int32_t> used;
    int32_t placed = 0;
    for (int32_t k = walk_off[i]; k < walk_off[i + 1]; ++k) {
      const kbg_fit_place& p = places[k];
      if (p.node < 0) {
        if (o.first_unplaced < 0) o.first_unplaced = p.task;
        continue;
      }
      (p.kind == KBG_KIND_ALLOCATE ? o.placed_idle : o.placed_releasing)++;
      used.push_back(p.node);
      ++placed;
      if (o.ready_after < 0 && o.ready_num + placed >= o.min_available) o.ready_after = k - walk_off[i] + 1;
    }
    std::sort(used.begin(), used.end());
    o.nodes_used = (int32_t)(std::unique(used.begin(), used.end()) - used.begin());
  }
  return KBG_OK;
}
