// kbg_node_why.ipp: which Pending tasks a node would take now.
// Part of kbg_session.cpp (one translation unit: included there inside its
// anonymous namespace, after kbg_job_fit.ipp; not compiled on its own).

// ============================================================ node reasons
// kbg_node_reasons: for any live node, every task that is Pending now under
// the cause kbg_task_reasons gives that node in the task's row (allocate.go:
// 119-162, backfill.go:50-64), against the session as it is now
// (kbg_device.hpp NodeWhy); nothing of the session changes.

kbg_status node_reasons(Session& S, const int32_t* nodes, int32_t n_nodes, kbg_node_why* out) {
  if (!S.opts.reasons) return fail(KBG_E_INVALID, "the session was opened without kbg_options.reasons");
  if (S.comm) return fail(KBG_E_UNSUPPORTED, "node reasons on a session over a communicator");
  if (!S.stream) return fail(KBG_E_UNSUPPORTED, "node reasons on a session without a device");
  if (n_nodes < 0 || (n_nodes > 0 && !out)) return fail(KBG_E_INVALID, "null argument");
  if (!nodes && n_nodes != S.n_nodes) return fail(KBG_E_INVALID, "nodes == NULL needs n_nodes == the node count");
  if (nodes)
    for (int32_t i = 0; i < n_nodes; ++i)
      if (nodes[i] < 0 || nodes[i] >= S.n_nodes) return fail(KBG_E_INVALID, "node index");
  if (n_nodes == 0) return KBG_OK;
  // before the cycle's first action the session is its snapshot
  const Engine& E = S.cycle_started ? S.fin : S.init;

  // one shape record per distinct key of the tasks that are Pending now
  // (task_reasons' key); the overused flag of a task's queue only splits the weight
  std::vector<kbg::NodeWhyShape> shapes;
  std::map<std::tuple<int32_t, int32_t, uint64_t, uint64_t, uint64_t>, int32_t> seen;
  auto bits = [](double v) {
    uint64_t u;
    std::memcpy(&u, &v, 8);
    return u;
  };
  std::vector<int8_t> q_over(S.n_queues, -1);
  int32_t pending = 0, last = -1;
  std::tuple<int32_t, int32_t, uint64_t, uint64_t, uint64_t> last_key{};
  for (int32_t t = 0; t < S.n_tasks; ++t) {
    if (!S.task_live[t]) continue;
    if ((S.cycle_started ? S.tstat[t] : (int32_t)S.tasks_in[t].status) != KBG_PENDING) continue;
    ++pending;
    const Res& r = S.treq[t];
    const int32_t be = kbg::res_empty(r) ? 1 : 0;
    const int32_t q = S.job_queue[S.task_job[t]];
    if (q_over[q] < 0) q_over[q] = S.has_prop && S.q_has_attr[q] && kbg::res_le(S.q_deserved[q], E.qalloc[q]) ? 1 : 0;
    const auto key = std::make_tuple(S.task_class[t], be, bits(r.c), bits(r.m), bits(r.g));
    if (last < 0 || key != last_key) {  // (a job's tasks mostly share a key: the map is asked once per run of them)
      auto [it, fresh] = seen.emplace(key, (int32_t)shapes.size());
      if (fresh)  // (the tasks ascend: the first of a key is its lowest)
        shapes.push_back({{S.task_class[t], be ? kbg::kTaskShapeBestEffort : 0, {r.c, r.m, r.g}}, 0, 0, t, 0});
      last = it->second;
      last_key = key;
    }
    kbg::NodeWhyShape& sh = shapes[last];
    sh.weight++;
    if (!q_over[q]) sh.weight_open++;
  }
  const int32_t Q = (int32_t)shapes.size();
  if (kbg_status st = ensure_stage_planes(S); st != KBG_OK) return st;
  const kbg::StagePlanes hp = kbg::kbg_stage_planes(S.h_stage.data(), S.n_classes, S.W);
  auto live = [&](int32_t n) { return (bool)((hp.live[n >> 6] >> (n & 63)) & 1ull); };
  for (int32_t i = 0; i < n_nodes; ++i) {
    const int32_t n = nodes ? nodes[i] : i;
    kbg_node_why& o = out[i];
    o = kbg_node_why{};
    if (!live(n)) continue;
    o.valid = 1;
    o.node = n;
    o.pending = pending;
    std::fill_n(o.first_task, KBG_TWHY_COUNT, -1);
  }
  if (Q == 0) return KBG_OK;
  // The device names the stage from the static planes alone; with host ports,
  // pod affinity or a nil Node it cannot: the whole table on the host.
  // KBG_HOST_NODE_WHY, read per call, asks for that on any session (A/B parity
  // tests, as KBG_HOST_TASK_WHY).
  const char* env = getenv("KBG_HOST_NODE_WHY");
  const bool host_only = S.has_ports || S.has_aff || S.any_nil || (env && env[0] == '1');
  if (host_only) {
    const kbg::AffState* aff = S.has_aff ? (S.cycle_started ? &S.affm->st : &S.affm->st0) : nullptr;
    std::vector<int32_t> done(S.n_nodes, -1);  // the first entry of `out` that holds a node's row
    for (int32_t i = 0; i < n_nodes; ++i) {
      kbg_node_why& o = out[i];
      if (!o.valid) continue;
      const int32_t n = o.node;
      if (done[n] >= 0) {
        o = out[done[n]];
        continue;
      }
      done[n] = i;
      for (const kbg::NodeWhyShape& sh : shapes) {
        const uint32_t key = host_task_why(S, hp, aff, sh.first_task, n);
        const int32_t c = (int32_t)(key & 0xffu);
        o.count[c] += sh.weight;
        if (o.first_task[c] < 0 || sh.first_task < o.first_task[c]) o.first_task[c] = sh.first_task;
        for (int d = 0; d < 3; ++d)
          if ((key >> (8 + d)) & 1u) o.idle_short[d] += sh.weight;
        if (c == KBG_TWHY_FITS_IDLE) {
          o.open_idle += sh.weight_open;
          if (sh.sh.flags & kbg::kTaskShapeBestEffort) o.idle_best_effort += sh.weight;
        } else if (c == KBG_TWHY_FITS_RELEASING) {
          o.open_releasing += sh.weight_open;
        }
      }
    }
    return KBG_OK;
  }

  kbg_status st;
  // node rows and mask words a victim action staged but has not pushed yet
  if (S.vt_ready && (!S.sdeltas.empty() || !S.mask_dirty.empty()))
    if ((st = victim_push(S, std::vector<int32_t>{})) != KBG_OK) return st;
  // the 64-node words of the table that hold a named live node, ascending
  const int32_t tab_words = (S.tab_n + 63) >> 6;
  std::vector<int32_t> words;
  if (!nodes) {
    words.resize(tab_words);
    std::iota(words.begin(), words.end(), 0);
  } else {
    for (int32_t i = 0; i < n_nodes; ++i)
      if (out[i].valid) words.push_back((nodes[i] - S.tab_lo) >> 6);
    std::sort(words.begin(), words.end());
    words.erase(std::unique(words.begin(), words.end()), words.end());
  }
  const int32_t NW = (int32_t)words.size();
  if (NW == 0) return KBG_OK;
  constexpr int32_t kChunk = 32768;  // shape records per launch (the grid's second dimension is their groups)
  const size_t scap = (size_t)std::min(Q, kChunk);
  auto drop = [&](void* p) {
    if (!p) return;
    pool_put(p);
    S.d_allocs.erase(std::find(S.d_allocs.begin(), S.d_allocs.end(), p));
  };
  if (S.nwhy_shape_cap < scap) {
    drop(S.d_nwhy_shapes);
    S.d_nwhy_shapes = nullptr;
    S.nwhy_shape_cap = 0;
    if ((st = dalloc(S, &S.d_nwhy_shapes, scap)) != KBG_OK) return st;
    S.nwhy_shape_cap = scap;
  }
  if (S.nwhy_word_cap < (size_t)NW) {
    drop(S.d_nwhy_words);
    drop(S.d_nwhy_out);
    S.d_nwhy_words = S.d_nwhy_out = nullptr;
    S.nwhy_word_cap = 0;
    const size_t wcap = (size_t)std::max(NW, std::min(tab_words, 16));
    if ((st = dalloc(S, &S.d_nwhy_words, wcap)) != KBG_OK) return st;
    if ((st = dalloc(S, &S.d_nwhy_out, wcap * 64 * kbg::kNodeWhyFields)) != KBG_OK) return st;
    S.nwhy_word_cap = wcap;
  }
  const int32_t P = NW * 64;  // the planes are packed: one copy brings the named words' slots back
  const kbg::StagePlanes dp = kbg::kbg_stage_planes(S.d_stage, S.n_classes, S.W);
  HIP_TRY(hipMemcpyAsync(S.d_nwhy_words, words.data(), (size_t)NW * sizeof(int32_t), hipMemcpyHostToDevice, S.stream));
  HIP_TRY(kbg::launch_node_why_init(S.d_nwhy_out, P, NW, S.stream));
  double why_ms = 0;  // event time of the kbg_node_why_kernel launches
  for (int32_t q0 = 0; q0 < Q; q0 += kChunk) {
    const int32_t nq = std::min(kChunk, Q - q0);
    HIP_TRY(hipMemcpyAsync(S.d_nwhy_shapes, shapes.data() + q0, (size_t)nq * sizeof(kbg::NodeWhyShape),
                           hipMemcpyHostToDevice, S.stream));
    const kbg::NodeWhyArgs a{S.d_nodes.idle_cpu, soa_stride(S), S.W,        S.tab_lo,       S.tab_n,
                             dp.sel_ok,          dp.taint_ok,   dp.unsched, dp.live,        S.d_nwhy_shapes,
                             nq,                 S.pred_active ? 1 : 0,     S.d_nwhy_words, NW,
                             P,                  S.d_nwhy_out};
    HIP_TRY(kbg::launch_node_why(a, S.stream, S.ev[0], S.ev[1]));
    // (the staging is reused by the next chunk: the launch that reads it ends first)
    HIP_TRY(hipStreamSynchronize(S.stream));
    if (S.tab_n > 0) {
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, S.ev[0], S.ev[1]));
      why_ms += ms;
    }
  }
  std::vector<int32_t> planes((size_t)P * kbg::kNodeWhyFields);
  HIP_TRY(hipMemcpyAsync(planes.data(), S.d_nwhy_out, planes.size() * sizeof(int32_t), hipMemcpyDeviceToHost, S.stream));
  HIP_TRY(hipStreamSynchronize(S.stream));
  S.vstage_busy = false;
  if (getenv("KBG_PROFILE_NODE_WHY"))
    fprintf(stderr, "[kbg node why] %d tasks, %d keys, %d words, why kernel %.3f ms\n", pending, Q, NW, why_ms);
  // the planes into rows
  for (int32_t i = 0; i < n_nodes; ++i) {
    kbg_node_why& o = out[i];
    if (!o.valid) continue;
    const int32_t row = o.node - S.tab_lo;
    const int32_t e = (int32_t)(std::lower_bound(words.begin(), words.end(), row >> 6) - words.begin());
    const int32_t* p = planes.data() + (size_t)e * 64 + (row & 63);
    for (int k = 0; k < kbg::kNodeWhyCauses; ++k) {
      o.count[kbg::kNodeWhyCause[k]] = p[(size_t)(kbg::kNwhyCount + k) * P];
      o.first_task[kbg::kNodeWhyCause[k]] = p[(size_t)(kbg::kNwhyFirst + k) * P];
    }
    for (int d = 0; d < 3; ++d) o.idle_short[d] = p[(size_t)(kbg::kNwhyShort + d) * P];
    o.open_idle = p[(size_t)kbg::kNwhyOpenIdle * P];
    o.open_releasing = p[(size_t)kbg::kNwhyOpenRel * P];
    o.idle_best_effort = p[(size_t)kbg::kNwhyIdleBestEffort * P];
  }
  return KBG_OK;
}
