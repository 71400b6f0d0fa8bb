// devmem_main.cpp -- the ownership rules of GmDevMem (shrimp_amd/csrc/gm_devmem.h), walked on the CPU.
//
// The holder is instantiated with a counting allocator that can be told to fail its k-th call (allocations, copies and host allocations all count).  walk() is shaped
// like a seam call: several get, several up (a null source and a zero count among them), one drop and re-get, a host buffer that grows, a second host buffer that is
// never handed over, an early return at the first failure, and give() on success only.  For k = 1..N (N = the calls of an undisturbed walk) the program checks after
// the walk: no live device allocation, nothing freed that was not live (freed twice, or freed again after drop), the host buffers freed unless given.
// Needs no GPU and no HIP: exit status 0 = all rules hold, otherwise one message per violation on stderr and status 1.
#define GM_DEVMEM_NO_HIP
#include "gm_devmem.h"
#include <cstdio>
#include <cstring>
#include <map>
#include <type_traits>

static int g_violations = 0;
#define EXPECT(cond, ...) do { if (!(cond)) { g_violations++; fprintf(stderr, "devmem: " __VA_ARGS__); fprintf(stderr, " [%s, k = %d]\n", #cond, CountAlloc::fail_at); } } while (0)

struct CountAlloc {
  typedef int error; typedef int stream; static constexpr error ok = 0;
  static int calls, fail_at, sync_copies, async_copies, releases;
  static std::map<void*, size_t> dev, host;                     // what is live, with its size
  static bool fails() { return ++calls == fail_at; }
  static void reset(int k) { calls = 0; fail_at = k; sync_copies = async_copies = releases = 0; }
  static error alloc(void** p, size_t bytes) { if (fails()) return 1; *p = malloc(bytes ? bytes : 1); dev[*p] = bytes; return ok; }
  static void release(void* p);
  static error copy(void* d, const void* h, size_t bytes, GmSyncCopy) { if (fails()) return 2; memcpy(d, h, bytes); sync_copies++; return ok; }
  static error copy(void* d, const void* h, size_t bytes, stream) { if (fails()) return 3; memcpy(d, h, bytes); async_copies++; return ok; }
  static void* host_alloc(void* old, size_t bytes, bool zeroed) {
    if (fails()) return nullptr;
    void* p = zeroed ? calloc(bytes, 1) : realloc(old, bytes);
    if (!zeroed && old) host.erase(old);
    host[p] = bytes; return p;
  }
  static void host_free(void* p);
};
int CountAlloc::calls, CountAlloc::fail_at, CountAlloc::sync_copies, CountAlloc::async_copies, CountAlloc::releases;
std::map<void*, size_t> CountAlloc::dev, CountAlloc::host;
void CountAlloc::release(void* p) { releases++; const bool live = dev.erase(p) == 1; EXPECT(live, "a device pointer is freed that is not live (twice, or again after drop)"); if (live) free(p); }
void CountAlloc::host_free(void* p) { const bool live = host.erase(p) == 1; EXPECT(live, "a host pointer is freed that is not live (twice, or after give)"); if (live) free(p); }

typedef GmDevMemT<CountAlloc> Mem;
static_assert(!std::is_copy_constructible<Mem>::value && !std::is_copy_assignable<Mem>::value, "the holder must not be copyable");

#define TRY(call) do { const int e_ = (call); if (e_ != CountAlloc::ok) return e_; } while (0)
// one seam call; *result: the buffer handed to the caller (on success only)
static int walk(char** result) {
  static const int src[8] = {1, 2, 3, 4, 5, 6, 7, 8};
  Mem mem;
  int *a = nullptr, *b = nullptr, *c = nullptr, *absent = nullptr, *empty = nullptr; unsigned char* scratch = nullptr; double* d = nullptr;
  TRY(mem.get(&a, 64));
  TRY(mem.get(&scratch, 100));
  TRY(mem.up(&b, src, 8, gm_sync, 32));                           // blocking copy, 32 bytes of room behind the array
  EXPECT(CountAlloc::dev.count(b) && CountAlloc::dev[b] == 8 * sizeof(int) + 32 && !memcmp(b, src, sizeof src), "up: size or content");
  TRY(mem.up(&c, src, 4, 7));                                     // asynchronous copy on "stream" 7
  { const int before = CountAlloc::calls;
    TRY(mem.up(&absent, nullptr, 8, 7)); TRY(mem.up(&empty, src, 0, gm_sync));
    EXPECT(!absent && !empty && CountAlloc::calls == before, "an absent array must leave the pointer null and allocate nothing"); }
  { const size_t live = CountAlloc::dev.size(); const int rel = CountAlloc::releases;
    mem.drop(scratch);
    EXPECT(!scratch && CountAlloc::dev.size() == live - 1 && CountAlloc::releases == rel + 1, "drop frees its buffer at once and clears the pointer");
    mem.drop(absent);                                             // (a null pointer: nothing happens)
    EXPECT(CountAlloc::releases == rel + 1, "drop of a null pointer frees nothing"); }
  TRY(mem.get(&scratch, 4000));                                   // the grown buffer in its place
  TRY(mem.get(&d, 16));
  char* text = mem.host(100, true);                               // zeroed
  if (!text) return -1;
  EXPECT(text[0] == 0 && text[99] == 0, "host(zeroed) is zeroed");
  memset(text, 'x', 100);
  char* scratch_host = mem.host(10);                              // a second host buffer, never handed over
  if (!scratch_host) return -1;
  { char* grown = mem.host(5000, false, text);                    // realloc growth; on failure the old buffer stays owned
    if (!grown) return -1;
    text = grown;
    EXPECT(text[0] == 'x' && text[99] == 'x', "a grown host buffer keeps its content"); }
  TRY(mem.up(&d, src, 2, 7));                                     // (a pointer taken twice: both buffers stay owned)
  EXPECT(CountAlloc::sync_copies == 1 && CountAlloc::async_copies == 2, "each up uses the copy its caller chose");
  *result = mem.give(text);
  return 0;
}

// the state after a walk: nothing live but the buffer that was given
static void check_after(int rc, char* result, bool want_ok) {
  EXPECT((rc == 0) == want_ok, "the walk returned %d", rc);
  EXPECT(CountAlloc::dev.empty(), "%zu device allocations are live after the call", CountAlloc::dev.size());
  if (rc == 0) {
    EXPECT(result && CountAlloc::host.size() == 1 && CountAlloc::host.count(result) == 1, "after success only the given host buffer lives (%zu do)", CountAlloc::host.size());
  } else {
    EXPECT(!result && CountAlloc::host.empty(), "after a failure no host buffer lives (%zu do)", CountAlloc::host.size());
    EXPECT(CountAlloc::calls == CountAlloc::fail_at, "the walk went on after its failure (%d calls)", CountAlloc::calls);
  }
  for (auto& kv : CountAlloc::dev) free(kv.first);
  for (auto& kv : CountAlloc::host) free(kv.first);              // (the caller's free of what it was given)
  CountAlloc::dev.clear(); CountAlloc::host.clear();
}

int main() {
  char* result = nullptr;
  CountAlloc::reset(0);                                           // undisturbed
  int rc = walk(&result);
  const int n_calls = CountAlloc::calls;
  check_after(rc, result, true);
  EXPECT(n_calls >= 12, "the undisturbed walk made %d allocator calls", n_calls);
  for (int k = 1; k <= n_calls; k++) {
    result = nullptr;
    CountAlloc::reset(k);
    rc = walk(&result);
    check_after(rc, result, false);
  }
  if (g_violations) { fprintf(stderr, "devmem: %d violations\n", g_violations); return 1; }
  printf("devmem ok: %d failure points walked, no leak, no double free\n", n_calls);
  return 0;
}
