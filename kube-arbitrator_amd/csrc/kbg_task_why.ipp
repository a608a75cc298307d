// kbg_task_why.ipp: why a Pending task would not be placed now.
// Part of kbg_session.cpp (one translation unit: included there inside its
// anonymous namespace, after kbg_victims.ipp; not compiled on its own).

// ============================================================ task reasons
// kbg_task_reasons: for any Pending task, every live node under the first
// cause that applies in the order of allocate.go:119-162 and backfill.go:50-64,
// against the session as it is now (kbg_device.hpp TaskWhy); nothing of the
// session changes.

// The cause of node n for task t on the host mirror, in the low byte, and for
// causes 7 and 8 the dimensions in which Idle.FitDelta(Resreq) is negative
// from bit 8. The predicate stage follows host_why: the current pod counts,
// ports and affinity state (`aff`: the live AffState, or the snapshot's before
// the cycle's first action). The node is live.
uint32_t host_task_why(Session& S, const kbg::StagePlanes& sp, const kbg::AffState* aff, int32_t t, int32_t n) {
  const int32_t cls = S.task_class[t];
  if (S.panic_node[n]) return KBG_TWHY_PANIC;  // predicates.go:122-123
  if (S.pred_active) {
    const size_t w = (size_t)cls * S.W + (n >> 6);
    const uint64_t bit = 1ull << (n & 63);
    if (S.ntasks[n] >= S.maxtasks[n]) return KBG_WHY_POD_CAP;
    if (!(sp.sel_ok[w] & bit)) return KBG_WHY_SELECTOR;
    if (S.has_ports)
      for (int32_t pw = 0; pw < S.PW; ++pw)
        if (S.node_ports[(size_t)n * S.PW + pw] & S.cls_conf[(size_t)cls * S.PW + pw]) return KBG_WHY_HOST_PORTS;
    if (sp.unsched[n >> 6] & bit) return KBG_WHY_UNSCHEDULABLE;
    if (!(sp.taint_ok[w] & bit)) return KBG_WHY_TAINTS;
    if (S.has_aff && !kbg::aff_ok(S, *aff, cls, n)) return KBG_WHY_POD_AFFINITY;
  }
  const Res& q = S.treq[t];
  if (kbg::res_empty(q)) return KBG_TWHY_FITS_IDLE;  // backfill.go:47-60: no resource test
  const Res& idle = S.idle[n];
  if (kbg::res_le(q, idle)) return KBG_TWHY_FITS_IDLE;
  uint32_t key = kbg::res_le(q, S.rel[n]) ? KBG_TWHY_FITS_RELEASING : KBG_TWHY_SHORT;
  // Resource.FitDelta (resource_info.go:116-129), kbg_fitdelta_kernel's expression
  if ((q.c > 0 ? idle.c - (q.c + kbg::kMinMilliCPU) : idle.c) < 0) key |= 1u << 8;
  if ((q.m > 0 ? idle.m - (q.m + kbg::kMinMemory) : idle.m) < 0) key |= 1u << 9;
  if ((q.g > 0 ? idle.g - (q.g + kbg::kMinMilliGPU) : idle.g) < 0) key |= 1u << 10;
  return key;
}

kbg_status task_reasons(Session& S, const int32_t* tasks, int32_t n_tasks, kbg_task_why* out) {
  if (!S.opts.reasons) return fail(KBG_E_INVALID, "the session was opened without kbg_options.reasons");
  if (S.comm) return fail(KBG_E_UNSUPPORTED, "task reasons on a session over a communicator");
  if (!S.stream) return fail(KBG_E_UNSUPPORTED, "task reasons on a session without a device");
  if (n_tasks < 0 || !tasks || (n_tasks > 0 && !out)) return fail(KBG_E_INVALID, "null argument");
  for (int32_t i = 0; i < n_tasks; ++i)
    if (tasks[i] < 0 || tasks[i] >= S.n_tasks) return fail(KBG_E_INVALID, "task index");
  if (n_tasks == 0) return KBG_OK;
  // before the cycle's first action the session is its snapshot
  const Engine& E = S.cycle_started ? S.fin : S.init;
  auto pending = [&](int32_t t) {
    if (!S.task_live[t]) return false;
    return (S.cycle_started ? S.tstat[t] : (int32_t)S.tasks_in[t].status) == KBG_PENDING;
  };

  // one device query per distinct key; a task's row is its key's
  std::vector<kbg::TaskShape> shapes;
  std::vector<int32_t> rep;  // a task of each key
  std::vector<int32_t> s_of(n_tasks, -1);
  std::map<std::tuple<int32_t, int32_t, uint64_t, uint64_t, uint64_t>, int32_t> seen;
  auto bits = [](double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return u;
  };
  for (int32_t i = 0; i < n_tasks; ++i) {
    const int32_t t = tasks[i];
    kbg_task_why& o = out[i];
    o = kbg_task_why{};
    if (!pending(t)) continue;
    o.valid = 1;
    o.task = t;
    const Res& r = S.treq[t];
    o.best_effort = kbg::res_empty(r) ? 1 : 0;
    const int32_t q = S.job_queue[S.task_job[t]];
    o.queue_overused = S.has_prop && S.q_has_attr[q] && kbg::res_le(S.q_deserved[q], E.qalloc[q]) ? 1 : 0;
    kbg::TaskShape sh{S.task_class[t], o.best_effort ? kbg::kTaskShapeBestEffort : 0, {r.c, r.m, r.g}};
    const auto key = std::make_tuple(sh.cls, sh.flags, bits(r.c), bits(r.m), bits(r.g));
    auto [it, fresh] = seen.emplace(key, (int32_t)shapes.size());
    if (fresh) {
      shapes.push_back(sh);
      rep.push_back(t);
    }
    s_of[i] = it->second;
  }
  const int32_t Q = (int32_t)shapes.size();
  if (Q == 0) return KBG_OK;
  if (kbg_status st = ensure_stage_planes(S); st != KBG_OK) return st;
  const kbg::StagePlanes hp = kbg::kbg_stage_planes(S.h_stage.data(), S.n_classes, S.W);
  std::vector<int32_t> rows((size_t)Q * kbg::kTaskWhyOut, 0);
  for (int32_t i = 0; i < Q; ++i)
    std::fill_n(rows.begin() + (size_t)i * kbg::kTaskWhyOut + kbg::kTwhyCauses, kbg::kTwhyCauses, -1);
  // The device names the stage from the static planes alone; with host ports,
  // pod affinity or a nil Node it cannot: the whole table on the host.
  // KBG_HOST_TASK_WHY, read per call, asks for that on any session (A/B parity
  // tests, as KBG_HOST_VICTIM_WHY).
  const char* env = getenv("KBG_HOST_TASK_WHY");
  const bool host_only = S.has_ports || S.has_aff || S.any_nil || (env && env[0] == '1');
  if (host_only) {
    const kbg::AffState* aff = S.has_aff ? (S.cycle_started ? &S.affm->st : &S.affm->st0) : nullptr;
    for (int32_t i = 0; i < Q; ++i) {
      int32_t* r = rows.data() + (size_t)i * kbg::kTaskWhyOut;
      for (int32_t n = 0; n < S.n_nodes; ++n) {
        if (!((hp.live[n >> 6] >> (n & 63)) & 1ull)) continue;
        const uint32_t key = host_task_why(S, hp, aff, rep[i], n);
        const int32_t c = (int32_t)(key & 0xffu);
        r[c]++;
        int32_t& first = r[kbg::kTwhyCauses + c];
        if (first < 0) first = n;  // (the nodes ascend)
        for (int d = 0; d < 3; ++d)
          if ((key >> (8 + d)) & 1u) r[2 * kbg::kTwhyCauses + d]++;
      }
    }
  } else {
    kbg_status st;
    // node rows and mask words a victim action staged but has not pushed yet
    if (S.vt_ready && (!S.sdeltas.empty() || !S.mask_dirty.empty()))
      if ((st = victim_push(S, std::vector<int32_t>{})) != KBG_OK) return st;
    constexpr int32_t kChunk = 32768;  // shapes per launch (the grid's second dimension is their groups)
    const size_t cap = (size_t)std::min(Q, kChunk);
    if (S.twhy_cap < cap) {
      for (void* p : {(void*)S.d_twhy_shapes, (void*)S.d_twhy_out})
        if (p) {
          pool_put(p);
          S.d_allocs.erase(std::find(S.d_allocs.begin(), S.d_allocs.end(), p));
        }
      S.d_twhy_shapes = nullptr;
      S.d_twhy_out = nullptr;
      S.twhy_cap = 0;
      if ((st = dalloc(S, &S.d_twhy_shapes, cap)) != KBG_OK) return st;
      if ((st = dalloc(S, &S.d_twhy_out, cap * kbg::kTaskWhyOut)) != KBG_OK) return st;
      S.twhy_cap = cap;
    }
    const kbg::StagePlanes dp = kbg::kbg_stage_planes(S.d_stage, S.n_classes, S.W);
    double why_ms = 0;  // event time of the kbg_task_why_kernel launches
    for (int32_t q0 = 0; q0 < Q; q0 += kChunk) {
      const int32_t nq = std::min(kChunk, Q - q0);
      HIP_TRY(hipMemcpyAsync(S.d_twhy_shapes, shapes.data() + q0, (size_t)nq * sizeof(kbg::TaskShape),
                             hipMemcpyHostToDevice, S.stream));
      const kbg::TaskWhyArgs a{S.d_nodes.idle_cpu, soa_stride(S), S.W,        S.tab_lo, S.tab_n,
                               dp.sel_ok,          dp.taint_ok,   dp.unsched, dp.live,  S.d_twhy_shapes,
                               nq,                 S.pred_active ? 1 : 0,     S.d_twhy_out};
      HIP_TRY(kbg::launch_task_why_init(S.d_twhy_out, nq, S.stream));
      HIP_TRY(kbg::launch_task_why(a, S.stream, S.ev[0], S.ev[1]));
      HIP_TRY(hipMemcpyAsync(rows.data() + (size_t)q0 * kbg::kTaskWhyOut, S.d_twhy_out,
                             (size_t)nq * kbg::kTaskWhyOut * sizeof(int32_t), hipMemcpyDeviceToHost, S.stream));
      HIP_TRY(hipStreamSynchronize(S.stream));
      if (S.tab_n > 0) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
        why_ms += ms;
      }
    }
    S.vstage_busy = false;
    if (getenv("KBG_PROFILE_TASK_WHY"))
      fprintf(stderr, "[kbg task why] %d tasks, %d keys, why kernel %.3f ms\n", n_tasks, Q, why_ms);
  }
  for (int32_t i = 0; i < n_tasks; ++i) {
    if (s_of[i] < 0) continue;
    const int32_t* r = rows.data() + (size_t)s_of[i] * kbg::kTaskWhyOut;
    kbg_task_why& o = out[i];
    for (int c = 0; c < KBG_TWHY_COUNT; ++c) {
      o.count[c] = r[c];
      o.first_node[c] = r[kbg::kTwhyCauses + c];
      o.visited += r[c];
    }
    for (int d = 0; d < 3; ++d) o.idle_short[d] = r[2 * kbg::kTwhyCauses + d];
  }
  return KBG_OK;
}
