// kbg_headroom.ipp: how many copies of a Pending task fit now.
// Part of kbg_session.cpp (one translation unit: included there inside its
// anonymous namespace, after kbg_task_why.ipp; not compiled on its own).

// ============================================================ task headroom
// kbg_task_headroom: for any Pending task, the copies each live node would
// take one after the other (kbg_device.hpp TaskRoom: LessEqual(Idle) then
// Idle.Sub, else LessEqual(Releasing) then Releasing.Sub, under the pod cap),
// summed over the nodes, against the session as it is now; nothing of the
// session changes.

// Node n for task t on the host mirror, added to row r (kRoomOut words). The
// predicate verdict is host_task_why's stage walk, the verdict of now, applied
// to every copy. A class with a host port holds one copy per node at most: the
// first copy's ports conflict with the second's (predicates.go:143-155), so its
// room is 1 wherever the pod cap leaves more. Returns false for a nil Node,
// which contributes nothing. The node is live.
bool host_headroom(Session& S, const kbg::StagePlanes& sp, const kbg::AffState* aff, int32_t t, int32_t n, int32_t limit,
                   int32_t* r) {
  const int32_t cls = S.task_class[t];
  if (S.panic_node[n]) return false;  // predicates.go:122-123
  int64_t room = INT32_MAX;
  if (S.pred_active) {
    const size_t w = (size_t)cls * S.W + (n >> 6);
    const uint64_t bit = 1ull << (n & 63);
    if (S.ntasks[n] >= S.maxtasks[n]) return true;
    if (!(sp.sel_ok[w] & bit)) return true;
    if (S.has_ports) {
      bool own = false;
      for (int32_t pw = 0; pw < S.PW; ++pw) {
        if (S.node_ports[(size_t)n * S.PW + pw] & S.cls_conf[(size_t)cls * S.PW + pw]) return true;
        own = own || S.cls_add[(size_t)cls * S.PW + pw] != 0;
      }
      if (own) room = 1;
    }
    if (sp.unsched[n >> 6] & bit) return true;
    if (!(sp.taint_ok[w] & bit)) return true;
    if (S.has_aff && !kbg::aff_ok(S, *aff, cls, n)) return true;
    room = std::min<int64_t>(room, (int64_t)S.maxtasks[n] - S.ntasks[n]);
  }
  r[kbg::kRoomNodesPass]++;
  const int32_t bound = (int32_t)std::min<int64_t>(limit, room);
  const Res& q = S.treq[t];
  int32_t i = 0, k_idle;
  if (kbg::res_empty(q)) {  // backfill.go:47-60: no resource test
    i = k_idle = bound;
  } else {
    Res a = S.idle[n];
    for (; i < bound && kbg::res_le(q, a); ++i) a.c -= q.c, a.m -= q.m, a.g -= q.g;  // node_info.go:108-118
    k_idle = i;
    Res b = S.rel[n];
    for (; i < bound && kbg::res_le(q, b); ++i) b.c -= q.c, b.m -= q.m, b.g -= q.g;  // node_info.go:119-126
  }
  r[kbg::kRoomCopiesIdle] += k_idle;
  r[kbg::kRoomCopiesRel] += i - k_idle;
  if (k_idle > 0) r[kbg::kRoomNodesIdle]++;
  if (k_idle == 0 && i > 0) r[kbg::kRoomNodesRelOnly]++;
  if (i > 0 && r[kbg::kRoomFirstNode] < 0) r[kbg::kRoomFirstNode] = n;  // (the nodes ascend)
  r[kbg::kRoomMaxNodeCopies] = std::max(r[kbg::kRoomMaxNodeCopies], i);
  if (i == limit && limit < room) r[kbg::kRoomLimitHit]++;
  return true;
}

kbg_status task_headroom(Session& S, const int32_t* tasks, int32_t n_tasks, int32_t limit, kbg_task_room* out) {
  if (!S.opts.reasons) return fail(KBG_E_INVALID, "the session was opened without kbg_options.reasons");
  if (S.comm) return fail(KBG_E_UNSUPPORTED, "task headroom on a session over a communicator");
  if (!S.stream) return fail(KBG_E_UNSUPPORTED, "task headroom on a session without a device");
  if (n_tasks < 0 || !tasks || (n_tasks > 0 && !out)) return fail(KBG_E_INVALID, "null argument");
  if (limit < 1 || limit > kbg::kRoomMaxLimit) return fail(KBG_E_INVALID, "limit outside 1..1024");
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
    kbg_task_room& o = out[i];
    o = kbg_task_room{};
    if (!pending(t)) continue;
    o.valid = 1;
    o.task = t;
    o.limit = limit;
    o.first_node = -1;
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
  if ((int64_t)S.n_nodes * limit > INT32_MAX) return fail(KBG_E_INVALID, "nodes * limit overflows a row's sums");
  if (kbg_status st = ensure_stage_planes(S); st != KBG_OK) return st;
  const kbg::StagePlanes hp = kbg::kbg_stage_planes(S.h_stage.data(), S.n_classes, S.W);
  std::vector<int32_t> rows((size_t)Q * kbg::kRoomOut, 0);
  for (int32_t i = 0; i < Q; ++i) rows[(size_t)i * kbg::kRoomOut + kbg::kRoomFirstNode] = -1;
  int32_t panic_nodes = 0;
  // The device knows the static stages alone; with host ports, pod affinity or
  // a nil Node the whole table is the host's. KBG_HOST_TASK_HEADROOM, read per
  // call, asks for that on any session (A/B parity tests, as KBG_HOST_TASK_WHY).
  const char* env = getenv("KBG_HOST_TASK_HEADROOM");
  const bool host_only = S.has_ports || S.has_aff || S.any_nil || (env && env[0] == '1');
  if (host_only) {
    const kbg::AffState* aff = S.has_aff ? (S.cycle_started ? &S.affm->st : &S.affm->st0) : nullptr;
    for (int32_t i = 0; i < Q; ++i) {
      int32_t* r = rows.data() + (size_t)i * kbg::kRoomOut;
      int32_t nil = 0;
      for (int32_t n = 0; n < S.n_nodes; ++n) {
        if (!((hp.live[n >> 6] >> (n & 63)) & 1ull)) continue;
        if (!host_headroom(S, hp, aff, rep[i], n, limit, r)) ++nil;
      }
      panic_nodes = nil;  // (the same for every key)
    }
  } else {
    kbg_status st;
    // node rows and mask words a victim action staged but has not pushed yet
    if (S.vt_ready && (!S.sdeltas.empty() || !S.mask_dirty.empty()))
      if ((st = victim_push(S, std::vector<int32_t>{})) != KBG_OK) return st;
    constexpr int32_t kChunk = 32768;  // shapes per launch (the grid's second dimension is their groups)
    const size_t cap = (size_t)std::min(Q, kChunk);
    if (S.room_cap < cap) {
      for (void* p : {(void*)S.d_room_shapes, (void*)S.d_room_out})
        if (p) {
          pool_put(p);
          S.d_allocs.erase(std::find(S.d_allocs.begin(), S.d_allocs.end(), p));
        }
      S.d_room_shapes = nullptr;
      S.d_room_out = nullptr;
      S.room_cap = 0;
      if ((st = dalloc(S, &S.d_room_shapes, cap)) != KBG_OK) return st;
      if ((st = dalloc(S, &S.d_room_out, cap * kbg::kRoomOut)) != KBG_OK) return st;
      S.room_cap = cap;
    }
    const kbg::StagePlanes dp = kbg::kbg_stage_planes(S.d_stage, S.n_classes, S.W);
    double room_ms = 0;  // event time of the kbg_task_headroom_kernel launches
    for (int32_t q0 = 0; q0 < Q; q0 += kChunk) {
      const int32_t nq = std::min(kChunk, Q - q0);
      HIP_TRY(hipMemcpyAsync(S.d_room_shapes, shapes.data() + q0, (size_t)nq * sizeof(kbg::TaskShape),
                             hipMemcpyHostToDevice, S.stream));
      const kbg::TaskRoomArgs a{S.d_nodes.idle_cpu, soa_stride(S), S.W,        S.tab_lo, S.tab_n,
                                dp.sel_ok,          dp.taint_ok,   dp.unsched, dp.live,  S.d_room_shapes,
                                nq,                 S.pred_active ? 1 : 0,     limit,    S.d_room_out};
      HIP_TRY(kbg::launch_task_headroom_init(S.d_room_out, nq, S.stream));
      HIP_TRY(kbg::launch_task_headroom(a, S.stream, S.ev[0], S.ev[1]));
      HIP_TRY(hipMemcpyAsync(rows.data() + (size_t)q0 * kbg::kRoomOut, S.d_room_out,
                             (size_t)nq * kbg::kRoomOut * sizeof(int32_t), hipMemcpyDeviceToHost, S.stream));
      HIP_TRY(hipStreamSynchronize(S.stream));
      if (S.tab_n > 0) {
        float ms = 0;
        HIP_TRY(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
        room_ms += ms;
      }
    }
    S.vstage_busy = false;
    if (getenv("KBG_PROFILE_TASK_HEADROOM"))
      fprintf(stderr, "[kbg task headroom] %d tasks, %d keys, limit %d, headroom kernel %.3f ms\n", n_tasks, Q, limit,
              room_ms);
  }
  for (int32_t i = 0; i < n_tasks; ++i) {
    if (s_of[i] < 0) continue;
    const int32_t* r = rows.data() + (size_t)s_of[i] * kbg::kRoomOut;
    kbg_task_room& o = out[i];
    o.copies_idle = r[kbg::kRoomCopiesIdle];
    o.copies_releasing = r[kbg::kRoomCopiesRel];
    o.nodes_idle = r[kbg::kRoomNodesIdle];
    o.nodes_releasing_only = r[kbg::kRoomNodesRelOnly];
    o.first_node = r[kbg::kRoomFirstNode];
    o.max_node_copies = r[kbg::kRoomMaxNodeCopies];
    o.nodes_pass = r[kbg::kRoomNodesPass];
    o.limit_hit = r[kbg::kRoomLimitHit];
    o.affinity_now = S.has_aff ? 1 : 0;
    o.panic_nodes = panic_nodes;
  }
  return KBG_OK;
}
