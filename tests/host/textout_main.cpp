// textout_main.cpp -- the rules of the ordered text buffer and its parked-buffer cache (shrimp_amd/csrc/gm_textout.h), walked on the CPU.
//
// Both are instantiated with a counting allocator that can be told to fail its k-th call.  A "call" is shaped like gm_map_reads: eight jobs of one to five pieces each,
// started in reverse order on threads of their own, append to one GmTextOut; the first job's pieces are small and the later ones large, so the first guess is too small
// and the buffer grows several times.  Checked: (a) the text is the pieces joined in job order, with its length and closing NUL; (b) with each allocator call failing in
// turn the call ends failed, every thread returns, nothing leaks and nothing is freed twice; (c) a job that fails instead of appending still passes the turn; (d) a
// buffer handed over is the caller's (capacity >= length + 1, not freed by the holder), one not handed over is freed by the holder; (e) a parked buffer that is large
// enough comes back as the next call's buffer, one that is too small is freed when the larger one is parked.
// Needs no GPU and no HIP: exit status 0 = all rules hold, otherwise one message per violation on stderr and status 1.
#include "gm_textout.h"
#include <cstdio>
#include <functional>
#include <map>
#include <thread>
#include <type_traits>

static std::atomic<int> g_violations(0);
#define EXPECT(cond, ...) do { if (!(cond)) { g_violations++; fprintf(stderr, "textout: " __VA_ARGS__); fprintf(stderr, " [%s, k = %d]\n", #cond, CountAlloc::fail_at); } } while (0)

struct CountAlloc {
  static std::mutex m; static int calls, fail_at; static std::map<void*, size_t> live;      // what is live, with its size
  static void reset(int k) { std::lock_guard<std::mutex> g(m); calls = 0; fail_at = k; }
  static void* grow(void* old, size_t bytes);
  static void release(void* p);
  static size_t size_of(void* p) { std::lock_guard<std::mutex> g(m); auto it = live.find(p); return it == live.end() ? 0 : it->second; }
  static size_t n_live() { std::lock_guard<std::mutex> g(m); return live.size(); }
};
std::mutex CountAlloc::m; int CountAlloc::calls, CountAlloc::fail_at; std::map<void*, size_t> CountAlloc::live;
void* CountAlloc::grow(void* old, size_t bytes) {
  std::lock_guard<std::mutex> g(m);
  if (++calls == fail_at) return nullptr;                         // (as realloc: the old block stays live)
  EXPECT(!old || live.count(old), "a block is grown that is not live");
  void* p = realloc(old, bytes ? bytes : 1);
  if (old) live.erase(old);
  live[p] = bytes; return p;
}
void CountAlloc::release(void* p) {
  if (!p) return;
  std::lock_guard<std::mutex> g(m);
  const bool was_live = live.erase(p) == 1; EXPECT(was_live, "a block is freed that is not live (twice, or after the hand-over)"); if (was_live) free(p);
}

typedef GmTextCacheT<CountAlloc> Cache;
typedef GmTextOutT<CountAlloc> Out;
static_assert(!std::is_copy_constructible<Out>::value && !std::is_copy_assignable<Out>::value, "the holder must not be copyable");

// fn on n threads at once (n - 1 new ones and the caller), as the library's thread pool runs it
static void run_on_threads(int n, const std::function<void()>& fn) { std::vector<std::thread> th; for (int t = 1; t < n; t++) th.emplace_back(fn); fn(); for (auto& t : th) t.join(); }

static const int N_JOBS = 8, UNITS = 10;
static std::atomic<int> g_copied(0);                             // pieces reported as copied
static std::vector<std::string> pieces_of(int j) {
  std::vector<std::string> v(1 + j % 5);
  for (size_t c = 0; c < v.size(); c++) v[c] = std::string(j == 0 ? 10 : 1200 + 37 * j + 5 * c, (char)('a' + (j * 5 + c) % 26)) + "\n";
  return v;
}
// One call.  fail_job: that job reports failure instead of appending; hand_over: ask for the text at the end.  Returns what hand_over gave (null: failed, or not asked).
static char* one_call(Cache& cache, size_t n_units, int fail_job, bool hand_over, size_t* len, bool* failed) {
  char* r = nullptr;
  {
    Out out(cache, n_units);
    std::vector<std::thread> th;
    for (int j = N_JOBS - 1; j >= 0; j--)
      th.emplace_back([&out, j, fail_job]() { if (j == fail_job) out.fail(j); else { const std::vector<std::string> p = pieces_of(j); out.append(j, p, UNITS, 3, run_on_threads, [](size_t) { g_copied++; }); } });
    for (auto& t : th) t.join();
    EXPECT(out.turn == N_JOBS, "after the last job the turn is %d", out.turn);
    *failed = out.failed;
    if (hand_over) { r = out.hand_over(len); EXPECT(!r || out.p == nullptr, "the holder keeps a buffer it handed over"); }
  }                                                               // (the holder frees what it still owns)
  return r;
}
static std::string expected_text() { std::string e; for (int j = 0; j < N_JOBS; j++) for (auto& p : pieces_of(j)) e += p; return e; }

int main() {
  const std::string want = expected_text();
  size_t len = 0; bool failed = false;
  { // (a), (d): the undisturbed call, handed over
    Cache cache; CountAlloc::reset(0);
    char* r = one_call(cache, N_JOBS * UNITS, -1, true, &len, &failed);
    const int n_calls = CountAlloc::calls;
    { int n_pieces = 0; for (int j = 0; j < N_JOBS; j++) n_pieces += (int)pieces_of(j).size(); EXPECT(g_copied == n_pieces, "%d of %d pieces were reported as copied", g_copied.load(), n_pieces); }
    EXPECT(r && !failed && len == want.size() && !memcmp(r, want.data(), len) && r[len] == 0, "the text is not the pieces joined in job order (%zu bytes, %zu expected)", len, want.size());
    EXPECT(n_calls >= 3, "the call made %d allocator calls: the buffer did not grow", n_calls);
    EXPECT(CountAlloc::n_live() == 1 && CountAlloc::size_of(r) >= len + 1, "after the hand-over the caller's buffer alone lives, with room for the NUL (%zu live)", CountAlloc::n_live());
    cache.give_back(r);                                           // (the caller's gm_free: too small to be parked)
    EXPECT(CountAlloc::n_live() == 0 && !cache.p, "a small buffer given back is freed, not parked");
    // (d) without a hand-over the holder frees its buffer
    r = one_call(cache, N_JOBS * UNITS, -1, false, &len, &failed);
    EXPECT(!r && !failed && CountAlloc::n_live() == 0, "a text that is not handed over is freed with the holder (%zu live)", CountAlloc::n_live());
    // (b) each allocator call fails in turn
    for (int k = 1; k <= n_calls; k++) {
      CountAlloc::reset(k);
      r = one_call(cache, N_JOBS * UNITS, -1, true, &len, &failed);
      EXPECT(failed && !r, "the call did not end failed");
      EXPECT(CountAlloc::calls == k, "the call went on allocating after its failure (%d calls)", CountAlloc::calls);
      EXPECT(CountAlloc::n_live() == 0, "%zu blocks are live after a failed call", CountAlloc::n_live());
    }
    // (c) a job that fails instead of appending: the others finish, the call is failed
    for (int j : {0, 3, N_JOBS - 1}) {
      CountAlloc::reset(0);
      r = one_call(cache, N_JOBS * UNITS, j, true, &len, &failed);
      EXPECT(failed && !r && CountAlloc::n_live() == 0, "job %d failed: the call must end failed with nothing live", j);
    }
    // the NUL of an empty text needs a block of its own, and that allocation may fail too
    for (int k = 0; k <= 1; k++) {
      CountAlloc::reset(k);
      { Out out(cache, 0); r = out.hand_over(&len); }
      EXPECT(k ? !r : (r && len == 0 && r[0] == 0), "an empty text is one NUL, or a failure");
      if (r) cache.give_back(r);
      EXPECT(CountAlloc::n_live() == 0, "the empty text leaks");
    }
  }
  { // (e) the parked buffer; n_units so large that the first guess passes the cache's 16 MB
    Cache cache; CountAlloc::reset(0);
    const size_t big = (size_t)20 << 20;
    char* r1 = one_call(cache, big, -1, true, &len, &failed);
    EXPECT(r1 && CountAlloc::size_of(r1) >= Cache::park_min && len == want.size(), "the first guess is %zu bytes", CountAlloc::size_of(r1));
    cache.give_back(r1);
    EXPECT(cache.p == r1 && CountAlloc::n_live() == 1, "a large buffer given back is parked");
    CountAlloc::reset(0);
    char* r2 = one_call(cache, big, -1, true, &len, &failed);
    EXPECT(r2 == r1 && CountAlloc::calls == 0 && !cache.p, "the parked buffer is the next call's buffer (%d allocator calls)", CountAlloc::calls);
    EXPECT(r2 && len == want.size() && !memcmp(r2, want.data(), len) && r2[len] == 0, "the text in the parked buffer");
    cache.give_back(r2);
    char* r3 = one_call(cache, 2 * big, -1, true, &len, &failed);  // twice the size: the parked one is too small and stays parked ...
    EXPECT(r3 && r3 != r1 && cache.p == r1 && CountAlloc::n_live() == 2, "a parked buffer that is too small must not be used");
    cache.give_back(r3);                                          // ... until the larger one comes back
    EXPECT(cache.p == r3 && CountAlloc::n_live() == 1 && CountAlloc::size_of(r1) == 0, "the smaller parked buffer is freed for the larger one (%zu live)", CountAlloc::n_live());
    cache.drop();
    EXPECT(CountAlloc::n_live() == 0 && !cache.p, "drop frees the parked buffer");
  }
  if (g_violations) { fprintf(stderr, "textout: %d violations\n", g_violations.load()); return 1; }
  printf("textout ok: order, failure points, failed jobs, hand-over and the parked buffer hold\n");
  return 0;
}
