// hostsim (developer tool, never shipped): replays a kbg_snapshot_save file
// through the session code on the simulated HIP stream, as a stand-alone
// program — the form the sanitizer builds take (make hostsim-tsan /
// hostsim-asan link the runtime into this executable).
//
//   hostsim_main SNAPSHOT OUT [--schedule eager|lazy] [--actions a,b,...]
//                [--batch-tasks N] [--candidates N] [--full-scan]
//                [--general-scan] [--repeat N] [--victim-reasons] [--job-fit]
//                [--node-why] [--drain]
//
// Each repeat opens a session, runs the actions (reclaim, allocate, backfill,
// preempt, in the order given), resets the session, runs them again and
// closes it. OUT receives, per run of the actions, the status of every call,
// the decision log (Allocate and Pipeline decisions) with the action behind
// each decision, the eviction log and every node's state as raw bytes, so two
// builds (or two schedules) are compared with cmp.
// --victim-reasons opens the session with kbg_options.reasons and calls
// kbg_victim_reasons for every job in all three modes after reclaim and after
// preempt. The rows do not go to OUT (the call changes nothing, so OUT is the
// same file with and without the flag); a summary goes to stderr.
// --job-fit opens the session with kbg_options.reasons too and calls
// kbg_job_fit for every job before the first action and after each one (once
// per action prefix), at limit 512 with the places and at limit 2 without. The
// rows do not go to OUT either; a summary goes to stderr.
// --node-why opens the session with kbg_options.reasons too and calls
// kbg_node_reasons before the first action and after each one, for every node
// and for a named subset (the last node, the first, the last again and every
// 70th: duplicates, out of order, one word or several). The rows do not go to
// OUT either; a summary goes to stderr.
// --drain opens the session with kbg_options.reasons too and calls
// kbg_node_drain before the first action and after each one: every node at
// limit 512 with the places and no cordon, then a named subset (the last node,
// the first, the last again and every 70th) at limit 2 without places, with
// every 3rd node cordoned. The rows do not go to OUT either; a summary goes to
// stderr.
// Exit status 0 unless the arguments or the files are unusable.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/kbgpu.h"

namespace {

void put(std::vector<char>& out, const void* p, size_t n) {
  out.insert(out.end(), (const char*)p, (const char*)p + n);
}
void put_i32(std::vector<char>& out, int32_t v) { put(out, &v, 4); }

kbg_status run_action(kbg_session* s, const std::string& a, kbg_decision* out, int32_t cap, int32_t* n) {
  if (a == "allocate") return kbg_allocate(s, out, cap, n);
  if (a == "backfill") return kbg_backfill(s, out, cap, n);
  if (a == "reclaim") return kbg_reclaim(s, out, cap, n);
  return kbg_preempt(s, out, cap, n);
}

// One run of the action list on an open session, through the C ABI calls the
// Python wrapper makes (kbgpu/actions.py): an action the reference would
// panic in (KBG_E_REF_PANIC) ends the list, and what the cycle logged up to
// there is still written.
// kbg_victim_reasons of every job in the three modes; what it found, to stderr.
void victim_reasons(kbg_session* s, const std::string& after, int32_t n_jobs) {
  std::vector<kbg_victim_why> why((size_t)n_jobs + 1);
  for (int32_t mode = KBG_VMODE_PREEMPT_JOBS; mode <= KBG_VMODE_RECLAIM; ++mode) {
    const kbg_status st = kbg_victim_reasons(s, mode, nullptr, n_jobs, why.data());
    if (st != KBG_OK) {
      fprintf(stderr, "hostsim_main: victim reasons after %s, mode %d: status %d: %s\n", after.c_str(), (int)mode,
              (int)st, kbg_last_error());
      continue;
    }
    int64_t valid = 0, count[KBG_VWHY_COUNT] = {}, fn[3] = {};
    for (int32_t j = 0; j < n_jobs; ++j) {
      if (!why[j].valid) continue;
      ++valid;
      for (int c = 0; c < KBG_VWHY_COUNT; ++c) count[c] += why[j].count[c];
      for (int f = 0; f < 3; ++f) fn[f] += why[j].fn_empty[f];
    }
    fprintf(stderr, "hostsim_main: victim reasons after %s, mode %d: %lld jobs with a Pending task; nodes per cause",
            after.c_str(), (int)mode, (long long)valid);
    for (int c = 0; c < KBG_VWHY_COUNT; ++c) fprintf(stderr, " %lld", (long long)count[c]);
    fprintf(stderr, "; fn_empty %lld %lld %lld\n", (long long)fn[0], (long long)fn[1], (long long)fn[2]);
  }
}

// kbg_job_fit of every job; what it found, to stderr.
void job_fit(kbg_session* s, const std::string& after, int32_t n_jobs) {
  std::vector<kbg_job_fit_row> rows((size_t)n_jobs + 1);
  int32_t need = 0;
  kbg_status st = kbg_job_fit(s, nullptr, n_jobs, 2, rows.data(), nullptr, 0, &need);
  std::vector<kbg_fit_place> places;
  if (st == KBG_OK && (st = kbg_job_fit(s, nullptr, n_jobs, KBG_FIT_MAX_LIMIT, rows.data(), nullptr, 0, &need)) == KBG_OK) {
    places.resize((size_t)need + 1);
    st = kbg_job_fit(s, nullptr, n_jobs, KBG_FIT_MAX_LIMIT, rows.data(), places.data(), need, &need);
  }
  if (st != KBG_OK) {
    fprintf(stderr, "hostsim_main: job fit after %s: status %d: %s\n", after.c_str(), (int)st, kbg_last_error());
    return;
  }
  int64_t valid = 0, idle = 0, rel = 0, nowhere = 0, ready = 0;
  for (int32_t j = 0; j < n_jobs; ++j) {
    if (!rows[j].valid) continue;
    ++valid;
    idle += rows[j].placed_idle;
    rel += rows[j].placed_releasing;
    ready += rows[j].ready_after >= 0;
    for (int32_t k = 0; k < rows[j].walked; ++k) nowhere += places[(size_t)rows[j].place_off + k].node < 0;
  }
  fprintf(stderr, "hostsim_main: job fit after %s: %lld jobs with a Pending task, %lld steps on idle, %lld on releasing, "
                  "%lld nowhere; %lld jobs get ready\n",
          after.c_str(), (long long)valid, (long long)idle, (long long)rel, (long long)nowhere, (long long)ready);
}

// kbg_node_reasons of every node and of a named subset; what it found, to stderr.
void node_why(kbg_session* s, const std::string& after, int32_t n_nodes) {
  std::vector<kbg_node_why> all((size_t)n_nodes + 1);
  std::vector<int32_t> pick;
  if (n_nodes > 0) pick = {n_nodes - 1, 0, n_nodes - 1};
  for (int32_t i = 70; i < n_nodes; i += 70) pick.push_back(i);
  std::vector<kbg_node_why> some(pick.size() + 1);
  kbg_status st = kbg_node_reasons(s, nullptr, n_nodes, all.data());
  if (st == KBG_OK) st = kbg_node_reasons(s, pick.data(), (int32_t)pick.size(), some.data());
  if (st != KBG_OK) {
    fprintf(stderr, "hostsim_main: node why after %s: status %d: %s\n", after.c_str(), (int)st, kbg_last_error());
    return;
  }
  int64_t valid = 0, pending = 0, count[KBG_TWHY_COUNT] = {}, open = 0, differ = 0;
  for (int32_t i = 0; i < n_nodes; ++i) {
    if (!all[i].valid) continue;
    ++valid;
    pending = all[i].pending;
    for (int c = 0; c < KBG_TWHY_COUNT; ++c) count[c] += all[i].count[c];
    open += all[i].open_idle + all[i].open_releasing;
  }
  for (size_t k = 0; k < pick.size(); ++k) differ += memcmp(&some[k], &all[pick[k]], sizeof(kbg_node_why)) != 0;
  fprintf(stderr, "hostsim_main: node why after %s: %lld live nodes, %lld Pending tasks; pairs per cause", after.c_str(),
          (long long)valid, (long long)pending);
  for (int c = 0; c < KBG_TWHY_COUNT; ++c) fprintf(stderr, " %lld", (long long)count[c]);
  fprintf(stderr, "; %lld open; %lld of %zu named rows differ\n", (long long)open, (long long)differ, pick.size());
}

// kbg_node_drain of every node, and of a named subset under a cordon; what it found, to stderr.
void node_drain(kbg_session* s, const std::string& after, int32_t n_nodes) {
  std::vector<kbg_node_drain_row> all((size_t)n_nodes + 1);
  std::vector<int32_t> pick, cordon;
  if (n_nodes > 0) pick = {n_nodes - 1, 0, n_nodes - 1};
  for (int32_t i = 70; i < n_nodes; i += 70) pick.push_back(i);
  for (int32_t i = 1; i < n_nodes; i += 3) cordon.push_back(i);
  std::vector<kbg_node_drain_row> some(pick.size() + 1);
  std::vector<kbg_fit_place> places;
  int32_t need = 0;
  kbg_status st = kbg_node_drain(s, nullptr, n_nodes, nullptr, 0, KBG_FIT_MAX_LIMIT, all.data(), nullptr, 0, &need);
  if (st == KBG_OK) {
    places.resize((size_t)need + 1);
    st = kbg_node_drain(s, nullptr, n_nodes, nullptr, 0, KBG_FIT_MAX_LIMIT, all.data(), places.data(), need, &need);
  }
  if (st == KBG_OK)
    st = kbg_node_drain(s, pick.data(), (int32_t)pick.size(), cordon.data(), (int32_t)cordon.size(), 2, some.data(),
                        nullptr, 0, &need);
  if (st != KBG_OK) {
    fprintf(stderr, "hostsim_main: node drain after %s: status %d: %s\n", after.c_str(), (int)st, kbg_last_error());
    return;
  }
  int64_t valid = 0, walked = 0, idle = 0, rel = 0, nowhere = 0, shrt = 0, cut = 0;
  for (int32_t i = 0; i < n_nodes; ++i) {
    if (!all[i].valid) continue;
    ++valid;
    walked += all[i].walked;
    idle += all[i].placed_idle;
    rel += all[i].placed_releasing;
    shrt += all[i].jobs_short;
    for (int32_t k = 0; k < all[i].walked; ++k) nowhere += places[(size_t)all[i].place_off + k].node < 0;
  }
  for (size_t k = 0; k < pick.size(); ++k) cut += some[k].valid ? some[k].unplaced : 0;
  fprintf(stderr, "hostsim_main: node drain after %s: %lld live nodes, %lld pods walked, %lld on idle, %lld on releasing, "
                  "%lld nowhere, %lld gangs short; %zu named rows under a cordon of %zu: %lld nowhere\n",
          after.c_str(), (long long)valid, (long long)walked, (long long)idle, (long long)rel, (long long)nowhere,
          (long long)shrt, pick.size(), cordon.size(), (long long)cut);
}

void run_actions(kbg_session* s, const std::vector<std::string>& actions, int32_t n_tasks, int32_t n_nodes,
                 std::vector<char>& out, int32_t why_jobs = -1, int32_t fit_jobs = -1, bool nwhy = false,
                 bool drain = false) {
  std::vector<kbg_decision> dec((size_t)n_tasks + 1);
  int32_t n = 0;
  if (fit_jobs >= 0) job_fit(s, "open", fit_jobs);
  if (nwhy) node_why(s, "open", n_nodes);
  if (drain) node_drain(s, "open", n_nodes);
  for (const std::string& a : actions) {
    const kbg_status st = run_action(s, a, dec.data(), (int32_t)dec.size(), &n);
    put_i32(out, (int32_t)st);
    if (st == KBG_E_REF_PANIC) break;
    if (st != KBG_OK) {
      fprintf(stderr, "hostsim_main: %s: status %d: %s\n", a.c_str(), (int)st, kbg_last_error());
      return;
    }
    if (why_jobs >= 0 && (a == "reclaim" || a == "preempt")) victim_reasons(s, a, why_jobs);
    if (fit_jobs >= 0) job_fit(s, a, fit_jobs);
    if (nwhy) node_why(s, a, n_nodes);
    if (drain) node_drain(s, a, n_nodes);
  }
  // the decision log (Allocate and Pipeline decisions of every action) and the action behind each
  put_i32(out, n);
  put(out, dec.data(), (size_t)n * sizeof(kbg_decision));
  std::vector<int32_t> acts((size_t)n + 1);
  int32_t na = 0;
  put_i32(out, (int32_t)kbg_decision_actions_get(s, acts.data(), (int32_t)acts.size(), &na));
  put_i32(out, na);
  put(out, acts.data(), (size_t)na * sizeof(int32_t));
  // the committed evictions of reclaim / preempt, in commit order
  int32_t ne = 0;
  put_i32(out, (int32_t)kbg_evictions_get(s, nullptr, 0, &ne));
  std::vector<kbg_eviction> ev((size_t)ne + 1);
  put_i32(out, (int32_t)kbg_evictions_get(s, ev.data(), ne, &ne));
  put_i32(out, ne);
  put(out, ev.data(), (size_t)ne * sizeof(kbg_eviction));
  for (int32_t i = 0; i < n_nodes; ++i) {
    kbg_node_state ns;
    memset(&ns, 0, sizeof ns);
    put_i32(out, (int32_t)kbg_node_state_get(s, i, &ns));
    put(out, &ns, sizeof ns);
  }
}

int usage() {
  fprintf(stderr,
          "usage: hostsim_main SNAPSHOT OUT [--schedule eager|lazy] [--actions reclaim,allocate,backfill,preempt]\n"
          "                    [--batch-tasks N] [--candidates N] [--full-scan] [--general-scan] [--repeat N]\n"
          "                    [--victim-reasons] [--job-fit] [--node-why] [--drain]\n"
          "  --actions: any of reclaim, allocate, backfill, preempt, run in the order given (default allocate)\n");
  return 2;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return usage();
  kbg_options opts;
  memset(&opts, 0, sizeof opts);
  std::vector<std::string> actions{"allocate"};
  int repeat = 1;
  bool why = false, fit = false, nwhy = false, drain = false;
  for (int i = 3; i < argc; ++i) {
    const std::string a = argv[i];
    const bool more = i + 1 < argc;
    if (a == "--schedule" && more) {
      setenv("KBG_HOSTSIM_SCHEDULE", argv[++i], 1);  // read at the simulator's first call
    } else if (a == "--actions" && more) {
      actions.clear();
      std::string list = argv[++i];
      for (size_t p = 0; p <= list.size();) {
        const size_t q = std::min(list.find(',', p), list.size());
        const std::string name = list.substr(p, q - p);
        if (name != "allocate" && name != "backfill" && name != "reclaim" && name != "preempt") {
          fprintf(stderr, "hostsim_main: unknown action %s (reclaim, allocate, backfill, preempt)\n", name.c_str());
          return 2;
        }
        actions.push_back(name);
        p = q + 1;
      }
    } else if (a == "--batch-tasks" && more) {
      opts.batch_tasks = atoi(argv[++i]);
    } else if (a == "--candidates" && more) {
      opts.candidates = atoi(argv[++i]);
    } else if (a == "--full-scan") {
      opts.full_scan = 1;
    } else if (a == "--general-scan") {
      setenv("KBG_FORCE_GENERAL_SCAN", "1", 1);
    } else if (a == "--victim-reasons") {
      why = true;
      opts.reasons = 1;
    } else if (a == "--job-fit") {
      fit = true;
      opts.reasons = 1;
    } else if (a == "--node-why") {
      nwhy = true;
      opts.reasons = 1;
    } else if (a == "--drain") {
      drain = true;
      opts.reasons = 1;
    } else if (a == "--repeat" && more) {
      repeat = atoi(argv[++i]);
    } else {
      return usage();
    }
  }
  kbg_snapshot_blob* blob = nullptr;
  if (kbg_snapshot_load(argv[1], &blob) != KBG_OK) {
    fprintf(stderr, "hostsim_main: %s: %s\n", argv[1], kbg_last_error());
    return 2;
  }
  const kbg_snapshot* snap = kbg_snapshot_blob_get(blob);
  std::vector<char> out;
  for (int r = 0; r < repeat; ++r) {
    kbg_session* s = nullptr;
    const kbg_status st = kbg_session_open(snap, &opts, &s);
    put_i32(out, (int32_t)st);
    if (st != KBG_OK) {
      fprintf(stderr, "hostsim_main: open: status %d: %s\n", (int)st, kbg_last_error());
      continue;
    }
    run_actions(s, actions, snap->n_tasks, snap->n_nodes, out, why ? snap->n_jobs : -1, fit ? snap->n_jobs : -1, nwhy,
                drain);
    const kbg_status rs = kbg_session_reset(s);
    put_i32(out, (int32_t)rs);
    if (rs == KBG_OK) run_actions(s, actions, snap->n_tasks, snap->n_nodes, out, why ? snap->n_jobs : -1, fit ? snap->n_jobs : -1, nwhy,
                drain);
    kbg_session_close(s);
  }
  kbg_snapshot_blob_free(blob);
  FILE* f = fopen(argv[2], "wb");
  if (!f || fwrite(out.data(), 1, out.size(), f) != out.size() || fclose(f) != 0) {
    fprintf(stderr, "hostsim_main: cannot write %s\n", argv[2]);
    return 2;
  }
  return 0;
}
