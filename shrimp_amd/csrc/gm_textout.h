// gm_textout.h -- the text a mapping call returns: one buffer that the call's host jobs append to in input order, and the cache that parks it between calls.  No HIP.
// The allocator is a template parameter for one reason: tests/host/textout_main.cpp walks the rules below on the CPU with a counting one.
#pragma once
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

struct GmCHeap { static void* grow(void* old, size_t bytes) { return realloc(old, bytes); } static void release(void* p) { free(p); } };
// The SAM text of a large call is hundreds of megabytes: allocating it afresh for every call (page faults on first touch) and unmapping it in gm_free cost 20+ ms per
// 1 M reads that nothing overlaps.  One freed text buffer of >= 16 MB is therefore parked here and handed to the next call (drop() frees it).
template <class A = GmCHeap> struct __attribute__((visibility("hidden"))) GmTextCacheT {      // (hidden, as GmDevMemT: no exports of the library)
  static constexpr size_t park_min = (size_t)16 << 20;
  std::mutex m; char* p = nullptr; size_t cap = 0; char* live = nullptr; size_t live_cap = 0;      // the parked buffer; the one the last call handed out
  // the parked buffer if it holds `want` bytes (a smaller one stays parked until a larger one comes back)
  char* take(size_t want, size_t* got) { std::lock_guard<std::mutex> g(m); if (!p || cap < want) return nullptr; char* r = p; *got = cap; p = nullptr; cap = 0; return r; }
  void track(char* r, size_t c) { std::lock_guard<std::mutex> g(m); live = r; live_cap = c; }
  // gm_free of a text buffer: the tracked one is parked when it is large and no larger one is parked already; everything else is freed
  void give_back(void* q) {
    { std::lock_guard<std::mutex> g(m);
      const bool mine = q == live; if (mine) live = nullptr;
      if (mine && live_cap >= park_min && !(p && cap >= live_cap)) { A::release(p); p = (char*)q; cap = live_cap; return; } }
    A::release(q);
  }
  void drop() { std::lock_guard<std::mutex> g(m); A::release(p); p = nullptr; cap = 0; }
};
// Job idx appends behind job idx - 1 (append waits for its turn), so the copy -- and the first touch of the output pages -- overlaps the device work instead of following
// it.  A job that cannot deliver calls fail(): the call ends failed and the turn still passes, so no later job waits for ever.  hand_over() gives the finished text to
// the caller; whatever was not handed over is freed with the holder.
template <class A = GmCHeap> struct __attribute__((visibility("hidden"))) GmTextOutT {
  GmTextCacheT<A>& cache; const size_t n_units;               // n_units: the reads of the whole call (the first guess scales a job's bytes per read by it)
  char* p = nullptr; size_t len = 0, cap = 0; int turn = 0; bool failed = false; std::mutex m; std::condition_variable cv;
  GmTextOutT(GmTextCacheT<A>& c, size_t n) : cache(c), n_units(n) {}
  ~GmTextOutT() { A::release(p); }
  // Job idx, which covers `units` of the call's n_units, appends its pieces; run(n, fn) runs fn on n threads at once and returns when all are done; copied(c) is called,
  // on one of them, as soon as piece c is in the buffer (the caller recycles its pieces while the others are still being copied).
  template <class Run, class Copied> void append(int idx, const std::vector<std::string>& pieces, size_t units, int nthreads, Run&& run, Copied&& copied) {
    std::vector<size_t> off(pieces.size()); size_t sz = 0; for (size_t c = 0; c < pieces.size(); c++) { off[c] = sz; sz += pieces[c].size(); }
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [&] { return turn == idx; });
    if (!failed && len + sz + 1 > cap) {
      // first guess: this job's bytes per read for all reads, then geometric growth (large blocks move by remapping)
      size_t want = std::max(len + sz + 1, cap + cap / 2);
      if (!cap) want = std::max(want, (size_t)((double)sz / std::max<size_t>(1, units) * 1.02 * n_units) + 4096);
      // the buffer of the last call, if it was given back and is about large enough: the first guess is an estimate (+- 1 % from one call to the next), a parked buffer just
      // below it would be thrown away for a fresh one (300 MB of page faults, ~25 ms a call on the calling thread's path), and a buffer that turns out short grows below anyway
      size_t ccap = 0; char* np = p ? nullptr : cache.take(std::max(len + sz + 1, want - want / 8), &ccap);
      if (np) want = ccap; else { if (!p) want += want / 16; np = (char*)A::grow(p, want); }
      if (!np) failed = true; else { p = np; cap = want; }
    }
    if (!failed) {
      char* dst = p + len; std::atomic<size_t> next(0);
      run(nthreads, [&]() { for (;;) { const size_t c = next.fetch_add(1); if (c >= pieces.size()) break; memcpy(dst + off[c], pieces[c].data(), pieces[c].size()); copied(c); } });
      len += sz;
    }
    turn = idx + 1; lk.unlock(); cv.notify_all();
  }
  // job idx has nothing to append (it failed): the call fails, the turn passes.  (Also after an append that did not get as far as passing it.)
  void fail(int idx) {
    std::unique_lock<std::mutex> lk(m);
    cv.wait(lk, [&] { return turn >= idx; });
    failed = true; if (turn == idx) turn = idx + 1;
    cv.notify_all();
  }
  // After the last job: the text to the caller, terminated with NUL and tracked for gm_free -- not shrunk: gm_free parks a large buffer for the next call.  Null when the
  // call failed or the terminator found no room; the holder then still owns (and frees) what it has.
  char* hand_over(size_t* text_len) {
    if (failed) return nullptr;
    if (!p || cap < len + 1) { char* r = (char*)A::grow(p, len + 1); if (!r) return nullptr; p = r; cap = len + 1; }
    char* r = p; p = nullptr; cache.track(r, cap); r[len] = 0; *text_len = len; return r;
  }
};
using GmTextOut = GmTextOutT<>;
