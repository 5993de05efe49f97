// Struct columns: their fields one after the other, or (two or more subtrees
// with launches of their own) forked over the context's side lanes (LaneFork
// does the events; what runs on which lane is decided here).
#include "reader_internal.hh"

int orcg_reader::decode_struct(uint32_t id, Col& c, const Rows& r) {
  std::vector<uint32_t> kids;
  size_t busy = 0;  // subtrees with launches of their own (the rest only wire batched outputs)
  for (uint32_t st : footer.types[id].subtypes)
    if (act.selected[st] && H->cols[st].supported) {
      kids.push_back(st);
      busy += device_work(st) ? 1 : 0;
    }
  // side streams only pay when at least two subtrees launch work
  const unsigned nl = in_lane || busy < 2 ? 1u : (unsigned)std::min<size_t>(num_lanes(), kids.size());
  if (nl > 1) return fork_struct(c, kids, nl, r);
  for (uint32_t st : kids) {
    const int rc = decode(st, r.n, c.nn, r.nonnull, r.rg_rows, c.nn ? r.d_nonnull : nullptr, &c);
    if (rc) return rc;
  }
  return ORCG_OK;
}

// Sibling subtrees on side streams (their kernels run concurrently: most
// launches of a stripe are one workgroup per row group, a fraction of the
// chip), forked after this column's work and joined back before anything
// reads their outputs (LaneFork: kid j on lane j % nl)
int orcg_reader::fork_struct(Col& c, const std::vector<uint32_t>& kids, unsigned nl, const Rows& r) {
  int rc = ORCG_OK;
  Ctx* base = act.ctx;
  if (!ctx_lane(base, 0)) return fail(ORCG_DEVICE_ERROR, "side stream creation failed");
  LaneFork lf(base);
  if ((rc = lf.begin())) return fail_ctx(rc);
  std::vector<Pending> level;  // lists / maps whose children wait for their element counts
  const Restore<std::vector<Pending>*> pending_scope(pending, &level);
  for (size_t j = 0; j < kids.size() && !rc; ++j) {
    Ctx* L = nullptr;
    if ((rc = lf.lane(j % nl, &L))) {
      rc = fail_ctx(rc);
      break;
    }
    const OnLane on_lane(this, L);
    rc = decode(kids[j], r.n, c.nn, r.nonnull, r.rg_rows, c.nn ? r.d_nonnull : nullptr, &c);
  }
  rc = fork_levels(lf, base, nl, level, rc);
  const int jr = lf.join();
  if (jr && !rc) rc = fail_ctx(jr);
  return rc;
}

// The fork's waiting children, level by level (rc: the first level's
// result). Within a level the subtrees with the most columns are enqueued
// first: the host's enqueue of a level takes longer than a short chain runs
// (configs[4]: the map's keys chain, the longest, started ~110 us late behind
// the list's items). Errors keep column order: after a failure only columns
// before it go on (their device errors would come first), the earliest
// column's failure is the one reported, and a level below keeps only the
// subtrees before it.
int orcg_reader::fork_levels(LaneFork& lf, Ctx* base, unsigned nl, std::vector<Pending>& level, int rc) {
  const int fork_rc = rc;
  const uint32_t fork_col = err_col;
  const std::string fork_msg = last_error;
  uint32_t fail_col = fork_rc ? fork_col : kNoCol;
  int fail_rc = fork_rc;
  std::string fail_msg = fork_rc ? fork_msg : std::string();
  int hard = ORCG_OK;  // a failure outside any column's decode: stop
  std::function<uint32_t(uint32_t)> cols_in = [&](uint32_t t) -> uint32_t {
    uint32_t k = act.selected[t] && H->cols[t].supported ? 1u : 0u;
    for (uint32_t st : footer.types[t].subtypes) k += cols_in(st);
    return k;
  };
  while (!level.empty() && !hard) {
    std::vector<Pending> cur;
    cur.swap(level);
    // below the first level `cur` is in weight-sorted enqueue order, not ascending ids
    size_t keep = 0;  // (pre-order: ascending ids)
    while (keep < cur.size() && cur[keep].id < fail_col) ++keep;
    cur.resize(keep);
    if (cur.empty()) break;
    std::vector<uint64_t> totals(cur.size(), 0);
    std::vector<CountSrc> srcs;
    for (const Pending& pd : cur) srcs.push_back(CountSrc{pd.lane, pd.d_total});
    if ((hard = read_back(srcs, totals.data()))) break;
    std::vector<uint32_t> weight(cur.size());
    std::vector<size_t> ord(cur.size());
    for (size_t q = 0; q < cur.size(); ++q) {
      weight[q] = cols_in(cur[q].id);
      ord[q] = q;
    }
    std::stable_sort(ord.begin(), ord.end(), [&](size_t x, size_t y) { return weight[x] > weight[y]; });
    for (size_t q : ord) {
      if (cur[q].id >= fail_col) continue;  // after an earlier failure
      // a map's keys and values are siblings too: when both launch work
      // the values go to the next lane of this fork, after what that lane
      // already holds (C5: the string keys' dictionary chain and the
      // nullable values' chain, ~190 + ~115 us, ran back to back on the
      // map's lane while the list's lane idled; a lane of its own would
      // share one of the process's 4 hardware queues, HIP's default)
      const std::vector<uint32_t>& subs = footer.types[cur[q].id].subtypes;
      std::vector<Ctx*> on(subs.size(), cur[q].lane);
      size_t li = 0;
      while (li < nl && base->lanes[li] != cur[q].lane) ++li;
      if (subs.size() == 2 && nl >= 2 && li < nl && device_work(subs[0]) && device_work(subs[1])) {
        const size_t alt = (li + 1) % nl;
        if ((hard = lf.chain(li, alt))) {
          hard = fail_ctx(hard);
          break;
        }
        on[1] = base->lanes[alt];
      }
      err_col = kNoCol;
      int lr = ORCG_OK;
      for (size_t si = 0; si < subs.size() && !lr; ++si) {
        const OnLane on_lane(this, on[si]);
        lr = decode(subs[si], totals[q], nullptr, totals[q], cur[q].child_rows);
      }
      if (lr) {
        const uint32_t ec = err_col != kNoCol ? err_col : cur[q].id;
        if (ec < fail_col) {
          fail_col = ec;
          fail_rc = lr;
          fail_msg = last_error;
        }
      }
    }
  }
  if (hard) {
    rc = hard;
  } else if (fail_rc) {
    rc = fail_rc;
    err_col = fail_col;
    last_error = fail_msg;
    act.ctx->last_error = fail_msg;
  }
  return rc;
}
