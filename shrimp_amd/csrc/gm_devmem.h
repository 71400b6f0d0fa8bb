// gm_devmem.h -- GmDevMem: the device and host memory of one seam call (or of one heavy-tier pass) under one owner.
//
// Rules.  Whatever get() / up() / host() handed out is freed when the holder leaves its scope, whichever return ends the call.  drop() frees one device buffer early and
// forgets it; give() hands a host buffer to the caller and forgets it.  To up(), an absent array -- a null source or a zero count -- is no error: the device pointer is
// left as it was (null).  The allocator is a template parameter for one reason: tests/host/devmem_main.cpp walks these rules on the CPU with a counting one.
#pragma once
#include <cstddef>
#include <cstdlib>
#include <vector>

struct GmSyncCopy {};                        // up(..., gm_sync): the blocking copy (null stream); up(..., stream): the asynchronous one on that stream
static constexpr GmSyncCopy gm_sync{};
struct GmHipAlloc;
#ifndef GM_DEVMEM_NO_HIP                     // (the CPU check brings its own allocator and no HIP)
struct GmHipAlloc {
  typedef hipError_t error; typedef hipStream_t stream; static constexpr error ok = hipSuccess;
  static error alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static void release(void* p) { (void)hipFree(p); }
  static error copy(void* d, const void* h, size_t bytes, GmSyncCopy) { return hipMemcpy(d, h, bytes, hipMemcpyHostToDevice); }
  static error copy(void* d, const void* h, size_t bytes, stream q) { return hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, q); }
  static void* host_alloc(void* old, size_t bytes, bool zeroed) { return zeroed ? calloc(bytes, 1) : realloc(old, bytes); }
  static void host_free(void* p) { free(p); }
};
#endif

template <class A = GmHipAlloc> struct __attribute__((visibility("hidden"))) GmDevMemT {      // (hidden: its instantiations are no exports of the library)
  typedef typename A::error error;
  GmDevMemT() { dev.reserve(16); }
  GmDevMemT(const GmDevMemT&) = delete; GmDevMemT& operator=(const GmDevMemT&) = delete;
  ~GmDevMemT() { for (void* p : dev) A::release(p); for (void* p : hst) A::host_free(p); }
  template <class T> error get(T** out, size_t bytes) { void* p = nullptr; const error e = A::alloc(&p, bytes); if (e == A::ok) { if (p) dev.push_back(p); *out = (T*)p; } return e; }
  // get + the copy of count elements from the host; pad_bytes: room behind them that is allocated and not written
  template <class T> error up(T** out, const void* src, size_t count, typename A::stream q, size_t pad_bytes = 0) { return up_(out, src, count, q, pad_bytes); }
  template <class T> error up(T** out, const void* src, size_t count, GmSyncCopy q, size_t pad_bytes = 0) { return up_(out, src, count, q, pad_bytes); }
  template <class T> void drop(T*& p) { for (void*& q : dev) if (p && q == (void*)p) { A::release(q); q = dev.back(); dev.pop_back(); break; } p = nullptr; }
  // a result buffer of the C heap: zeroed (calloc), or old -- one of this holder's -- grown as realloc grows it.  Null when out of memory: old then stays owned.
  template <class T = char> T* host(size_t bytes, bool zeroed = false, T* old = nullptr) {
    void* p = A::host_alloc(old, bytes, zeroed); if (!p) return nullptr;
    for (void*& q : hst) if (old && q == (void*)old) { q = p; return (T*)p; }
    hst.push_back(p); return (T*)p;
  }
  template <class T> T* give(T* p) { for (void*& q : hst) if (q == (void*)p) { q = hst.back(); hst.pop_back(); break; } return p; }
 private:
  std::vector<void*> dev, hst;
  template <class T, class Q> error up_(T** out, const void* src, size_t count, Q q, size_t pad_bytes) {
    if (!src || !count) return A::ok;
    const error e = get(out, count * sizeof(T) + pad_bytes);
    return e == A::ok ? A::copy((void*)*out, src, count * sizeof(T), q) : e;
  }
};
using GmDevMem = GmDevMemT<>;
