// gm_fasta.hip -- genome FASTA text -> the resident 4-bit bitfield, packed on the device (the first half of load_genome, ref: gmapper/genome.c:1050-1124
// with the reader of common/fasta.c:316-553 in letter space).
//
// Host: I/O only.  A reader thread fills pinned chunks (read(), or gzread() for a gzip file); the calling thread hands every chunk to the device on a copy
// stream of its own and, one chunk behind, reads the few words the kernels left: the bases so far, the first bad byte, one record per '>' line.  It cuts the
// contig names out of the chunk it still holds.  It never walks sequence bytes.
// Device, per chunk (tiles of FA_TILE bytes, one workgroup each, 16 bytes per lane):
//   k_fasta_tiles   what a tile does to the stream whatever comes before it: has it a line start, the kind of its last line, the sequence bytes it holds before
//                   its first line start (kept only when the line that reaches into it is a sequence line) and after it, its '>' lines
//   k_fasta_scan    one workgroup: exclusive scan of those records from the state the previous chunk left on the device -> per tile the kind of the incoming
//                   line, the bases and the '>' lines before it; leaves the state for the next chunk
//   k_fasta_pack    classifies again with the incoming kind known, ranks the kept bytes (wave prefix + carry across the waves), translates them through a
//                   256-entry table in LDS, compacts the 4-bit codes in LDS and writes whole words; the first and the last word of a tile are shared with
//                   its neighbours and go out with one atomicOr each into the zero-initialised bitfield
// The kind of a line comes from its first byte ('>' header, '#' comment, anything else sequence); a byte is kept when its line is a sequence line and it is
// not the '\n'.  Lines longer than the reference's 8 MiB line buffer (which it would cut into pieces and classify piece by piece) are out of scope.
#include <algorithm>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>
#include <zlib.h>
#include "gm_common.h"
#include "gm_internal.h"

#define FA_TPB 256
#define FA_TILE (FA_TPB * 16)
enum { FA_SEQ = 0, FA_HDR = 1, FA_CMT = 2, FA_UNKNOWN = 3 };

// what crosses a chunk edge (device memory, one per build), and what the host reads after every chunk
struct FaState {
  unsigned long long bases;        // bases emitted so far (after the chunk)
  unsigned long long chunk_base;   // ... before the chunk
  unsigned long long bad;          // offset in the chunk of the first byte of a sequence line that is no letter (~0: none)
  uint32_t kind;                   // kind of the line the chunk's last byte belongs to
  uint32_t prev_nl;                // the chunk's last byte was '\n'
  uint32_t n_hdr;                  // '>' lines of the chunk
  uint32_t prev_nl_in;             // prev_nl as the chunk found it (k_fasta_pack runs after k_fasta_scan has moved prev_nl on)
};
struct FaTile { uint32_t has_last; uint32_t before, after, n_hdr; };       // has_last: bit 0 = a line starts in the tile, bits 1..2 = kind of the last such line
struct FaTileIn { uint32_t kind, hdr_base, bases_rel, pad; };             // the line that reaches into the tile; '>' lines / bases of the chunk before the tile
struct FaHdr { uint32_t off, bases_rel; };                                // a '>' at chunk offset off, after bases_rel bases of the chunk

struct FaLane { uint32_t nl, st, hd, cm, valid; };                          // 16-bit masks over the lane's bytes: '\n', line start, '>' / '#' at a line start, inside the chunk
__device__ __forceinline__ uint32_t fa_byte(const uint4& v, int j) { const uint32_t w = j < 4 ? v.x : j < 8 ? v.y : j < 12 ? v.z : v.w; return (w >> ((j & 3) * 8)) & 0xffu; }
__device__ __forceinline__ FaLane fa_lane(const uint8_t* __restrict__ chunk, uint32_t n, uint32_t g0, const uint4& v, uint32_t first_prev_nl) {
  FaLane L; L.nl = L.st = L.hd = L.cm = L.valid = 0;
  uint32_t prev = g0 == 0 ? first_prev_nl : (g0 <= n ? (uint32_t)(chunk[g0 - 1] == '\n') : 0u);
#pragma unroll
  for (int j = 0; j < 16; j++) {
    const uint32_t b = fa_byte(v, j), in = (g0 + j < n) ? 1u : 0u, isnl = in & (uint32_t)(b == '\n');
    L.valid |= in << j; L.nl |= isnl << j;
    const uint32_t st = in & prev;
    L.st |= st << j; L.hd |= (st & (uint32_t)(b == '>')) << j; L.cm |= (st & (uint32_t)(b == '#')) << j;
    prev = isnl;
  }
  return L;
}
__device__ __forceinline__ uint32_t fa_last_kind(const FaLane& L) { const uint32_t top = 31u - __clz(L.st); return (L.hd >> top) & 1u ? FA_HDR : ((L.cm >> top) & 1u ? FA_CMT : FA_SEQ); }
// sequence bytes of the lane: those of lines whose kind is not known yet (before the first line start, with in == FA_UNKNOWN) and the known ones
__device__ __forceinline__ void fa_count(const FaLane& L, uint32_t in, uint32_t* before, uint32_t* after) {
  const uint32_t body = L.valid & ~L.nl;
  uint32_t seq_from_start = 0, cur = FA_UNKNOWN;           // bytes from the first line start on that belong to sequence lines
#pragma unroll
  for (int j = 0; j < 16; j++) {
    if ((L.st >> j) & 1u) cur = (L.hd >> j) & 1u ? FA_HDR : ((L.cm >> j) & 1u ? FA_CMT : FA_SEQ);
    seq_from_start |= (uint32_t)(cur == FA_SEQ) << j;
  }
  const uint32_t head = L.st ? ((L.st & (0u - L.st)) - 1u) : 0xffffu;        // the bytes before the first line start
  const uint32_t nhead = __popc(body & head), ntail = __popc(body & seq_from_start);
  if (in == FA_UNKNOWN) { *before = nhead; *after = ntail; } else { *before = 0; *after = ntail + (in == FA_SEQ ? nhead : 0u); }
}
// the kind of the line that reaches into this lane, from the lanes of its wave (FA_UNKNOWN: from before the wave); *w_has / *w_last: the wave's own
__device__ __forceinline__ uint32_t fa_wave_in(const FaLane& L, int lane, uint32_t* w_has, uint32_t* w_last) {
  const uint32_t last = L.st ? fa_last_kind(L) : 0u;
  const unsigned long long H = __ballot(L.st != 0);
  const unsigned long long lower = H & ((1ull << lane) - 1ull);
  const int p = lower ? 63 - __clzll((long long)lower) : 0;
  const uint32_t lp = (uint32_t)__shfl((int)last, p);
  const uint32_t lw = (uint32_t)__shfl((int)last, H ? 63 - __clzll((long long)H) : 0);
  *w_has = H ? 1u : 0u; *w_last = lw;
  return lower ? lp : (uint32_t)FA_UNKNOWN;
}
__device__ __forceinline__ uint32_t fa_wave_sum(uint32_t x) { for (int d = 32; d > 0; d >>= 1) x += (uint32_t)__shfl_xor((int)x, d); return x; }

__global__ void __launch_bounds__(FA_TPB) k_fasta_tiles(const uint8_t* __restrict__ chunk, uint32_t n, const FaState* __restrict__ st, int file_start, FaTile* __restrict__ tiles) {
  __shared__ uint32_t s_has[4], s_last[4], s_before[4], s_after[4], s_hdr[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t g0 = blockIdx.x * FA_TILE + threadIdx.x * 16;
  const uint4 v = *(const uint4*)(chunk + g0);                                     // (the chunk buffer is a whole number of tiles)
  const FaLane L = fa_lane(chunk, n, g0, v, file_start ? 1u : st->prev_nl);
  uint32_t w_has, w_last, before, after;
  const uint32_t in = fa_wave_in(L, lane, &w_has, &w_last);
  fa_count(L, in, &before, &after);
  before = fa_wave_sum(before); after = fa_wave_sum(after);
  const uint32_t nh = fa_wave_sum(__popc(L.hd));
  if (lane == 0) { s_has[wave] = w_has; s_last[wave] = w_last; s_before[wave] = before; s_after[wave] = after; s_hdr[wave] = nh; }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t has = 0, last = 0, bf = 0, af = 0, h = 0;
    for (int w = 0; w < 4; w++) {
      if (has) af += s_after[w] + (last == FA_SEQ ? s_before[w] : 0u); else { bf += s_before[w]; af = s_after[w]; }
      if (s_has[w]) { has = 1; last = s_last[w]; }
      h += s_hdr[w];
    }
    FaTile t; t.has_last = has | (last << 1); t.before = bf; t.after = af; t.n_hdr = h;
    tiles[blockIdx.x] = t;
  }
}

__global__ void __launch_bounds__(FA_TPB) k_fasta_scan(const uint8_t* __restrict__ chunk, uint32_t n, FaState* __restrict__ st, int file_start, const FaTile* __restrict__ tiles,
                                                       uint32_t n_tiles, FaTileIn* __restrict__ tin) {
  __shared__ uint32_t s_has[FA_TPB], s_last[FA_TPB], s_before[FA_TPB], s_after[FA_TPB], s_hdr[FA_TPB];
  __shared__ uint32_t s_kind[FA_TPB], s_bases[FA_TPB], s_hbase[FA_TPB];
  const uint32_t per = (n_tiles + FA_TPB - 1) / FA_TPB, t0 = threadIdx.x * per, t1 = min(n_tiles, t0 + per);
  { uint32_t has = 0, last = 0, bf = 0, af = 0, h = 0;
    for (uint32_t t = t0; t < t1; t++) {
      const FaTile T = tiles[t];
      if (has) af += T.after + (last == FA_SEQ ? T.before : 0u); else { bf += T.before; af = T.after; }
      if (T.has_last & 1u) { has = 1; last = T.has_last >> 1; }
      h += T.n_hdr;
    }
    s_has[threadIdx.x] = has; s_last[threadIdx.x] = last; s_before[threadIdx.x] = bf; s_after[threadIdx.x] = af; s_hdr[threadIdx.x] = h; }
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t kind = file_start ? (uint32_t)FA_SEQ : st->kind, bases = 0, h = 0;
    for (int i = 0; i < FA_TPB; i++) {
      s_kind[i] = kind; s_bases[i] = bases; s_hbase[i] = h;
      bases += s_after[i] + (kind == FA_SEQ ? s_before[i] : 0u);
      if (s_has[i]) kind = s_last[i];
      h += s_hdr[i];
    }
    const unsigned long long b0 = st->bases;
    st->prev_nl_in = file_start ? 1u : st->prev_nl;
    st->chunk_base = b0; st->bases = b0 + bases; st->kind = kind; st->n_hdr = h; st->bad = ~0ull;
    st->prev_nl = n ? (uint32_t)(chunk[n - 1] == '\n') : (file_start ? 1u : st->prev_nl);
  }
  __syncthreads();
  uint32_t kind = s_kind[threadIdx.x], bases = s_bases[threadIdx.x], h = s_hbase[threadIdx.x];
  for (uint32_t t = t0; t < t1; t++) {
    const FaTile T = tiles[t];
    FaTileIn I; I.kind = kind; I.hdr_base = h; I.bases_rel = bases; I.pad = 0;
    tin[t] = I;
    bases += T.after + (kind == FA_SEQ ? T.before : 0u);
    if (T.has_last & 1u) kind = T.has_last >> 1;
    h += T.n_hdr;
  }
}

__global__ void __launch_bounds__(FA_TPB) k_fasta_pack(const uint8_t* __restrict__ chunk, uint32_t n, FaState* __restrict__ st, int file_start, const FaTileIn* __restrict__ tin,
                                                       uint32_t* __restrict__ genome, unsigned long long cap_words, FaHdr* __restrict__ hdrs, uint32_t hdr_cap) {
  __shared__ uint8_t s_tab[256];
  __shared__ uint32_t s_words[FA_TILE / 8 + 8];
  __shared__ uint32_t s_has[4], s_last[4], s_cnt[4], s_nhdr, s_bad;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  { // fasta_open's letter-space table (ref: common/fasta.c:165-199): A C G T U M R W S Y K V H D B N -> 0..15, X and '.' -> 15, either case; 0xff: no letter
    const char* up = "ACGTUMRWSYKVHDBN"; const int c = threadIdx.x; uint8_t code = 0xff;
    for (int k = 0; k < 16; k++) if (c == up[k] || c == (up[k] | 0x20)) code = (uint8_t)k;
    if (c == 'X' || c == 'x' || c == '.') code = 15;
    s_tab[c] = code; }
  for (int i = threadIdx.x; i < FA_TILE / 8 + 8; i += FA_TPB) s_words[i] = 0;
  if (threadIdx.x == 0) { s_nhdr = 0; s_bad = 0xffffffffu; }
  const uint32_t g0 = blockIdx.x * FA_TILE + threadIdx.x * 16;
  const uint4 v = *(const uint4*)(chunk + g0);
  const FaLane L = fa_lane(chunk, n, g0, v, file_start ? 1u : st->prev_nl_in);
  uint32_t w_has, w_last;
  uint32_t in = fa_wave_in(L, lane, &w_has, &w_last);
  if (lane == 0) { s_has[wave] = w_has; s_last[wave] = w_last; }
  __syncthreads();
  const FaTileIn I = tin[blockIdx.x];
  if (in == FA_UNKNOWN) { in = I.kind; for (int w = 0; w < wave; w++) if (s_has[w]) in = s_last[w]; }
  // the lane's kept bytes as 4-bit codes, in order
  unsigned long long acc = 0; uint32_t cnt = 0, bad = 0xffffffffu, cur = in;
#pragma unroll
  for (int j = 0; j < 16; j++) {
    if ((L.st >> j) & 1u) cur = (L.hd >> j) & 1u ? FA_HDR : ((L.cm >> j) & 1u ? FA_CMT : FA_SEQ);
    if (cur == FA_SEQ && ((L.valid & ~L.nl) >> j) & 1u) {
      const uint32_t code = s_tab[fa_byte(v, j)];
      if (code == 0xffu) bad = min(bad, g0 + j);
      acc |= (unsigned long long)(code & 15u) << (4 * cnt); cnt++;
    }
  }
  // exclusive rank of the lane's first kept byte within the tile
  uint32_t incl = cnt;
  for (int d = 1; d < 64; d <<= 1) { const uint32_t up = (uint32_t)__shfl_up((int)incl, d); if (lane >= d) incl += up; }
  if (lane == 63) s_cnt[wave] = incl;
  __syncthreads();
  uint32_t rank = incl - cnt, total = 0;
  for (int w = 0; w < 4; w++) { if (w < wave) rank += s_cnt[w]; total += s_cnt[w]; }
  const unsigned long long P0 = st->chunk_base + I.bases_rel;                    // global position of the tile's first base
  const uint32_t q0 = (uint32_t)(P0 & 7ull);
  if (cnt) {
    const uint32_t q = q0 + rank, sh = (q & 7u) * 4u, w = q >> 3;
    const unsigned long long lo = acc << sh, hi = sh ? acc >> (64u - sh) : 0ull;
    if ((uint32_t)lo) atomicOr(&s_words[w], (uint32_t)lo);
    if ((uint32_t)(lo >> 32)) atomicOr(&s_words[w + 1], (uint32_t)(lo >> 32));
    if ((uint32_t)hi) atomicOr(&s_words[w + 2], (uint32_t)hi);
  }
  if (bad != 0xffffffffu) atomicMin(&s_bad, bad);
  // one record per '>' line (rare: the lanes that hold one walk their bytes again); the order within a tile is free, the host sorts by offset
  if (L.hd) {
    uint32_t c2 = 0, cur2 = in;
    for (int j = 0; j < 16; j++) {
      if ((L.st >> j) & 1u) {
        cur2 = (L.hd >> j) & 1u ? FA_HDR : ((L.cm >> j) & 1u ? FA_CMT : FA_SEQ);
        if (cur2 == FA_HDR) {
          const uint32_t slot = I.hdr_base + atomicAdd(&s_nhdr, 1u);
          if (slot < hdr_cap) { FaHdr h; h.off = g0 + j; h.bases_rel = I.bases_rel + rank + c2; hdrs[slot] = h; }
        }
      }
      if (cur2 == FA_SEQ && ((L.valid & ~L.nl) >> j) & 1u) c2++;
    }
  }
  __syncthreads();
  if (total) {
    const uint32_t nw = (q0 + total + 7u) >> 3;
    const unsigned long long W0 = P0 >> 3;
    for (uint32_t i = threadIdx.x; i < nw; i += FA_TPB) {
      const uint32_t x = s_words[i];
      if (W0 + i >= cap_words) continue;                                           // (never with the capacity the host keeps; a bound, not a path)
      if (i == 0 || i == nw - 1) { if (x) atomicOr(&genome[W0 + i], x); }          // shared with the neighbouring tiles
      else genome[W0 + i] = x;
    }
  }
  if (threadIdx.x == 0 && s_bad != 0xffffffffu) atomicMin(&st->bad, (unsigned long long)s_bad);
}

// ---- host: I/O and the few words per chunk --------------------------------------------------------------------------------------------------------------
namespace {
constexpr int FA_SLOTS = 3;                        // chunks in flight: one being read, one on its way to / on the device, one whose names the host cuts out
constexpr size_t FA_HDR_EAGER = 1024;              // '>' records fetched with the state words; a chunk with more of them costs one more copy

struct FaSlot {
  uint8_t* h = nullptr; uint8_t* d = nullptr; FaHdr* d_hdr = nullptr; FaTile* d_tiles = nullptr; FaTileIn* d_tin = nullptr;
  struct Res { FaState st; FaHdr hdr[FA_HDR_EAGER]; }* res = nullptr;        // pinned
  hipEvent_t copied = nullptr, done = nullptr;
  size_t n = 0; int file = 0; uint64_t file_off = 0; bool first = false, last = false, io_error = false;
  int owner = 0;                                  // 0: the reader's to fill, 1: filled, the caller's
};

struct FaBuild {                                   // everything the call owns; the destructor runs on every path out of it
  size_t chunk = 0; uint32_t hdr_cap = 0;
  FaSlot slot[FA_SLOTS];
  hipStream_t s_copy = nullptr, s_kern = nullptr;
  FaState* d_state = nullptr; uint32_t* d_genome = nullptr; uint64_t cap_words = 0;
  std::thread reader; std::mutex m; std::condition_variable cv; bool stop = false;
  ~FaBuild() {
    { std::lock_guard<std::mutex> lk(m); stop = true; } cv.notify_all();
    if (reader.joinable()) reader.join();
    if (s_kern) (void)hipStreamSynchronize(s_kern);
    if (s_copy) (void)hipStreamSynchronize(s_copy);
    for (FaSlot& S : slot) {
      if (S.h) (void)hipHostFree(S.h); if (S.res) (void)hipHostFree(S.res);
      (void)hipFree(S.d); (void)hipFree(S.d_hdr); (void)hipFree(S.d_tiles); (void)hipFree(S.d_tin);
      if (S.copied) (void)hipEventDestroy(S.copied); if (S.done) (void)hipEventDestroy(S.done);
    }
    (void)hipFree(d_state); (void)hipFree(d_genome);
    if (s_copy) (void)hipStreamDestroy(s_copy); if (s_kern) (void)hipStreamDestroy(s_kern);
  }
};

// the reader thread: every file in order, chunk by chunk into the slots in turn
void fa_reader(FaBuild* B, int n_files, const char* const* paths) {
  int k = 0;
  for (int f = 0; f < n_files; f++) {
    int fd = open(paths[f], O_RDONLY);
    gzFile gz = nullptr;
    if (fd >= 0) {
      unsigned char magic[2] = {0, 0};
      if (pread(fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b) { gz = gzdopen(fd, "rb"); if (gz) gzbuffer(gz, 1 << 20); else { close(fd); fd = -1; } }
    }
    uint64_t off = 0; bool first = true;
    for (;;) {
      FaSlot& S = B->slot[k];
      { std::unique_lock<std::mutex> lk(B->m); B->cv.wait(lk, [&] { return B->stop || S.owner == 0; }); if (B->stop) { if (gz) gzclose(gz); else if (fd >= 0) close(fd); return; } }
      size_t n = 0; bool err = fd < 0, eof = err;
      while (!eof && n < B->chunk) {
        const size_t want = std::min<size_t>(B->chunk - n, 1u << 30);
        const long got = gz ? (long)gzread(gz, S.h + n, (unsigned)want) : (long)read(fd, S.h + n, want);
        if (got < 0) { err = true; break; }
        if (got == 0) {                                  // a gzip stream that ends early gives no negative count: zlib hands out what it could inflate, then 0 with Z_BUF_ERROR
          if (gz) { int zerr = Z_OK; (void)gzerror(gz, &zerr); if (zerr != Z_OK && zerr != Z_STREAM_END) { err = true; break; } }
          eof = true;
        }
        n += (size_t)got;
      }
      S.n = n; S.file = f; S.file_off = off; S.first = first; S.last = eof || err; S.io_error = err;
      off += n; first = false;
      { std::lock_guard<std::mutex> lk(B->m); S.owner = 1; } B->cv.notify_all();
      k = (k + 1) % FA_SLOTS;
      if (eof || err) break;
    }
    if (gz) gzclose(gz); else if (fd >= 0) close(fd);
  }
}
}  // namespace

int gm_fasta_to_device(int n_files, const char* const* paths, GmFastaGenome* out) {
  FaBuild B;
  B.chunk = (size_t)32 << 20;
  if (const char* e = gm_tune("GM_FASTA_CHUNK")) B.chunk = (size_t)std::max(64ll, std::min(1ll << 30, atoll(e)));
  B.hdr_cap = (uint32_t)(B.chunk / 4 + 16);
  const size_t chunk_alloc = (B.chunk + FA_TILE - 1) / FA_TILE * FA_TILE, max_tiles = chunk_alloc / FA_TILE;
  // the bitfield is sized from the file sizes: a plain file holds at least as many bytes as bases; a gzip file is guessed at four times its size and the bitfield
  // grows geometrically (device-to-device copy) when the text turns out longer.  Never beyond 2^32 bases and the chunks in flight: such a genome fails below.
  uint64_t guess = 0;
  for (int f = 0; f < n_files; f++) {
    struct stat sb;
    if (!paths[f] || stat(paths[f], &sb) != 0) { gm_set_error("cannot open genome file '%s'", paths[f] ? paths[f] : "(null)"); return GM_E_ARG; }
    unsigned char magic[2] = {0, 0}; const int fd = open(paths[f], O_RDONLY);
    if (fd < 0) { gm_set_error("cannot open genome file '%s'", paths[f]); return GM_E_ARG; }
    const bool gz = pread(fd, magic, 2, 0) == 2 && magic[0] == 0x1f && magic[1] == 0x8b; close(fd);
    guess += (uint64_t)sb.st_size * (gz ? 4u : 1u);
  }
  const uint64_t limit_bases = (1ull << 32) + (uint64_t)FA_SLOTS * B.chunk;
  auto words_for = [](uint64_t bases) { return bases / 8 + 64 + 2; };
  B.cap_words = words_for(std::min(guess, limit_bases));
  GM_HIP(hipStreamCreateWithFlags(&B.s_copy, hipStreamNonBlocking));
  GM_HIP(hipStreamCreateWithFlags(&B.s_kern, hipStreamNonBlocking));
  GM_HIP(hipMalloc(&B.d_genome, B.cap_words * 4));
  GM_HIP(hipMemsetAsync(B.d_genome, 0, B.cap_words * 4, B.s_kern));
  GM_HIP(hipMalloc(&B.d_state, sizeof(FaState)));
  GM_HIP(hipMemsetAsync(B.d_state, 0, sizeof(FaState), B.s_kern));
  for (FaSlot& S : B.slot) {
    GM_HIP(hipHostMalloc((void**)&S.h, chunk_alloc, hipHostMallocDefault));
    GM_HIP(hipHostMalloc((void**)&S.res, sizeof(FaSlot::Res), hipHostMallocDefault));
    GM_HIP(hipMalloc(&S.d, chunk_alloc));
    GM_HIP(hipMemsetAsync(S.d, '\n', chunk_alloc, B.s_kern));                       // (the bytes behind a chunk's end are masked by index; defined all the same)
    GM_HIP(hipMalloc(&S.d_hdr, (size_t)B.hdr_cap * sizeof(FaHdr)));
    GM_HIP(hipMalloc(&S.d_tiles, max_tiles * sizeof(FaTile)));
    GM_HIP(hipMalloc(&S.d_tin, max_tiles * sizeof(FaTileIn)));
    GM_HIP(hipEventCreateWithFlags(&S.copied, hipEventDisableTiming));
    GM_HIP(hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
  }
  GM_HIP(hipStreamSynchronize(B.s_kern));
  B.reader = std::thread(fa_reader, &B, n_files, paths);

  // per-contig results, and the host's own state across chunks: the header line that has not ended yet, the start of the current file
  std::vector<uint64_t> starts; std::vector<std::string> names; std::vector<int> contig_file;
  std::string open_hdr; bool hdr_open = false, file_started = false, in_comment = false;
  uint64_t submitted = 0, bases = 0; int rc = GM_OK;
  auto finish_name = [&](int file) -> int {                                          // open_hdr: the header line without its '\n'
    if (open_hdr.size() <= 1) { gm_set_error("genome file '%s': contig %zu has an empty header line", paths[file], names.size() + 1); return GM_E_ARG; }
    names.push_back(gm_extract_name(open_hdr)); hdr_open = false; open_hdr.clear();
    return GM_OK;
  };
  auto process = [&](FaSlot& S) -> int {                                             // the chunk's kernels are done
    const FaState& st = S.res->st; const uint8_t* p = S.h; const char* path = paths[S.file];
    if (S.first) { file_started = false; in_comment = false; }
    if (S.io_error) { gm_set_error("cannot read genome file '%s' to its end (read error, or a truncated or damaged gzip stream)", path); return GM_E_ARG; }
    const size_t begun_before = starts.size();
    // the file must begin with a '>' line ('#' lines may stand before it): the reference stops reading such a file and goes on without it
    size_t i = 0;
    while (!file_started && i < S.n) {
      if (in_comment) { const void* e = memchr(p + i, '\n', S.n - i); if (!e) { i = S.n; break; } i = (size_t)((const uint8_t*)e - p) + 1; in_comment = false; continue; }
      if (p[i] == '#') { in_comment = true; continue; }
      if (p[i] == '>') { file_started = true; break; }
      gm_set_error("genome file '%s' does not start with a '>' line (byte %llu is 0x%02x)", path, (unsigned long long)(S.file_off + i), p[i]); return GM_E_ARG;
    }
    if (st.n_hdr > B.hdr_cap) { gm_set_error("genome file '%s': more than %u header lines in %zu bytes", path, B.hdr_cap, S.n); return GM_E_ARG; }
    std::vector<FaHdr> hdr(S.res->hdr, S.res->hdr + std::min<size_t>(st.n_hdr, FA_HDR_EAGER));
    if (st.n_hdr > FA_HDR_EAGER) { hdr.resize(st.n_hdr); GM_HIP(hipMemcpy(hdr.data(), S.d_hdr, (size_t)st.n_hdr * sizeof(FaHdr), hipMemcpyDeviceToHost)); }
    std::sort(hdr.begin(), hdr.end(), [](const FaHdr& a, const FaHdr& b) { return a.off < b.off; });
    if (hdr_open) {                                                                  // a header line that began in an earlier chunk
      const void* e = memchr(p, '\n', S.n);
      open_hdr.append((const char*)p, e ? (size_t)((const uint8_t*)e - p) : S.n);
      if (e) { const int r = finish_name(S.file); if (r) return r; }
    }
    for (const FaHdr& h : hdr) {
      if (hdr_open) { gm_set_error("genome file '%s': internal error, a header inside a header line", path); return GM_E_ARG; }
      starts.push_back(st.chunk_base + h.bases_rel); contig_file.push_back(S.file);
      const void* e = memchr(p + h.off, '\n', S.n - h.off);
      open_hdr.assign((const char*)p + h.off, e ? (size_t)((const uint8_t*)e - (p + h.off)) : S.n - h.off);
      hdr_open = true;
      if (e) { const int r = finish_name(S.file); if (r) return r; }
    }
    if (st.bad != ~0ull) {
      // the contig the byte stands in: the last header before it
      size_t c = begun_before; for (const FaHdr& h : hdr) if (h.off < st.bad) c++;
      const std::string nm = c >= 1 && c - 1 < names.size() ? names[c - 1] : std::string("?");
      gm_set_error("genome file '%s': invalid sequence; tag: [%s]: byte 0x%02x at offset %llu is no nucleotide letter", path, nm.c_str(), p[st.bad], (unsigned long long)(S.file_off + st.bad));
      return GM_E_ARG;
    }
    bases = st.bases;
    if (bases >= (1ull << 32)) { gm_set_error("genome of %llu bp exceeds the reference's 32-bit global coordinates", (unsigned long long)bases); return GM_E_ARG; }
    if (S.last) {
      if (!file_started) { gm_set_error("genome file '%s' holds no contig", path); return GM_E_ARG; }
      if (hdr_open) { gm_set_error("genome file '%s' ends inside a header line", path); return GM_E_ARG; }
      if (starts.back() == bases) { gm_set_error("genome file '%s': contig [%s] had no sequence", path, names.back().c_str()); return GM_E_ARG; }
    }
    return GM_OK;
  };

  int k = 0, prev = -1; bool all_read = false; int files_done = 0;
  while (!all_read || prev >= 0) {
    int cur = -1;
    if (!all_read) {
      FaSlot& S = B.slot[k];
      { std::unique_lock<std::mutex> lk(B.m); B.cv.wait(lk, [&] { return S.owner == 1; }); }
      cur = k; k = (k + 1) % FA_SLOTS;
      if (S.last && ++files_done == n_files) all_read = true;
      if (S.io_error && S.n == 0 && S.first) { gm_set_error("cannot open genome file '%s'", paths[S.file]); rc = GM_E_ARG; }
      // room for every base this chunk can hold
      submitted += S.n;
      const uint64_t need = words_for(std::min(submitted, limit_bases));
      if (rc == GM_OK && need > B.cap_words) {
        const uint64_t grown = std::min(std::max(need, B.cap_words * 2), words_for(limit_bases));
        uint32_t* g2 = nullptr;
        GM_HIP(hipStreamSynchronize(B.s_kern));
        GM_HIP(hipMalloc(&g2, grown * 4));
        hipError_t e1 = hipMemsetAsync(g2 + B.cap_words, 0, (grown - B.cap_words) * 4, B.s_kern);
        hipError_t e2 = hipMemcpyAsync(g2, B.d_genome, B.cap_words * 4, hipMemcpyDeviceToDevice, B.s_kern);
        hipError_t e3 = hipStreamSynchronize(B.s_kern);
        if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) { (void)hipFree(g2); gm_set_error("growing the genome bitfield failed"); return GM_E_NODEVICE; }
        (void)hipFree(B.d_genome); B.d_genome = g2; B.cap_words = grown;
      }
      if (rc == GM_OK && S.n) {
        const uint32_t n = (uint32_t)S.n, tiles = (uint32_t)((S.n + FA_TILE - 1) / FA_TILE);
        GM_HIP(hipMemcpyAsync(S.d, S.h, S.n, hipMemcpyHostToDevice, B.s_copy));
        GM_HIP(hipEventRecord(S.copied, B.s_copy));
        GM_HIP(hipStreamWaitEvent(B.s_kern, S.copied, 0));
        hipLaunchKernelGGL(k_fasta_tiles, dim3(tiles), dim3(FA_TPB), 0, B.s_kern, S.d, n, B.d_state, S.first ? 1 : 0, S.d_tiles);
        hipLaunchKernelGGL(k_fasta_scan, dim3(1), dim3(FA_TPB), 0, B.s_kern, S.d, n, B.d_state, S.first ? 1 : 0, S.d_tiles, tiles, S.d_tin);
        hipLaunchKernelGGL(k_fasta_pack, dim3(tiles), dim3(FA_TPB), 0, B.s_kern, S.d, n, B.d_state, S.first ? 1 : 0, S.d_tin, B.d_genome, (unsigned long long)B.cap_words, S.d_hdr, B.hdr_cap);
        GM_HIP(hipGetLastError());
        GM_HIP(hipMemcpyAsync(&S.res->st, B.d_state, sizeof(FaState), hipMemcpyDeviceToHost, B.s_kern));
        GM_HIP(hipMemcpyAsync(S.res->hdr, S.d_hdr, sizeof(FaHdr) * std::min<size_t>(FA_HDR_EAGER, B.hdr_cap), hipMemcpyDeviceToHost, B.s_kern));
        GM_HIP(hipEventRecord(S.done, B.s_kern));
      }
    }
    if (prev >= 0) {                                                                 // the chunk before: its words are in (or about to be), this one's copy is under way
      FaSlot& S = B.slot[prev];
      if (S.n) { GM_HIP(hipEventSynchronize(S.done)); if (rc == GM_OK) rc = process(S); }
      else if (rc == GM_OK) {                                                       // an empty read: the end of a file whose size is a multiple of the chunk, or an empty file
        if (S.io_error) { gm_set_error("cannot read genome file '%s' to its end (read error, or a truncated or damaged gzip stream)", paths[S.file]); rc = GM_E_ARG; }
        else if (S.first || !file_started) { gm_set_error("genome file '%s' holds no contig", paths[S.file]); rc = GM_E_ARG; }
        else if (hdr_open) { gm_set_error("genome file '%s' ends inside a header line", paths[S.file]); rc = GM_E_ARG; }
        else if (starts.back() == bases) { gm_set_error("genome file '%s': contig [%s] had no sequence", paths[S.file], names.back().c_str()); rc = GM_E_ARG; }
      }
      { std::lock_guard<std::mutex> lk(B.m); S.owner = 0; } B.cv.notify_all();
    }
    if (rc != GM_OK) return rc;
    prev = cur;
  }
  // contig table; an empty contig in the middle shows as two equal starts
  const size_t nc = starts.size();
  if (nc == 0 || names.size() != nc) { gm_set_error("no contig in the genome files"); return GM_E_ARG; }
  { const int r = gm_refuse_contig_count("gm_index_build_fasta", nc); if (r != GM_OK) return r; }          // (the bitfield and the slots go with B)
  out->names = names; out->lens.resize(nc);
  for (size_t c = 0; c < nc; c++) {
    const uint64_t end = c + 1 < nc ? starts[c + 1] : bases;
    if (end == starts[c]) { gm_set_error("genome file '%s': contig [%s] had no sequence", paths[contig_file[c]], names[c].c_str()); return GM_E_ARG; }
    out->lens[c] = (uint32_t)(end - starts[c]);
  }
  // hand over a bitfield of (total + 7) / 8 + 64 words, everything behind the last base zero: the one the text was packed into when it is at most an eighth
  // larger than that (plain files: about 1.5 % for 70-column lines), otherwise a copy of exactly that size (gzip files whose size was guessed)
  const uint64_t words = (bases + 7) / 8 + 64;
  uint32_t* g = nullptr;
  if (B.cap_words <= words + words / 8) { GM_HIP(hipStreamSynchronize(B.s_kern)); g = B.d_genome; B.d_genome = nullptr; }
  else {
    GM_HIP(hipMalloc(&g, words * 4));
    if (hipMemcpyAsync(g, B.d_genome, words * 4, hipMemcpyDeviceToDevice, B.s_kern) != hipSuccess || hipStreamSynchronize(B.s_kern) != hipSuccess) {
      (void)hipFree(g); gm_set_error("copying the genome bitfield failed"); return GM_E_NODEVICE;
    }
  }
  out->d_genome = g; out->words = words; out->total = bases;
  return GM_OK;
}
