// hostio.hpp -- the transfer engine between host memory or files and HBM (hostio.hip): chunked streams through the context's two
// pinned buffers, whole files in and out, and output files whose own pages the copy engine writes (MappedOut).
#pragma once
#include "kernels.hpp"
#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdlib>
#include <mutex>
#include <fcntl.h>
#include <unistd.h>
#include <sys/mman.h>
#include <sys/vfs.h>

namespace pfp __attribute__((visibility("hidden"))) {      // (internal to the library: not among its exported symbols)

// host bytes -> device, (fd, file offset) -> device (parallel pread), device -> host bytes: each returns once the host side is
// done with its buffer; the last host -> device chunk may still be crossing PCIe on the context's stream
void upload(pfp_ctx *c, uint8_t *d_dst, const void *src, uint64_t nbytes);
void upload_fd(pfp_ctx *c, uint8_t *d_dst, int fd, uint64_t file_off, uint64_t nbytes);
void download(pfp_ctx *c, void *dst, const uint8_t *d_src, uint64_t nbytes);
// a text given as a host pointer or, where that is null, as bytes [file_off, file_off + nbytes) of an open file
inline void upload_text(pfp_ctx *c, uint8_t *d_dst, const uint8_t *text, int fd, uint64_t file_off, uint64_t nbytes) {
  if (text) upload(c, d_dst, text, nbytes); else upload_fd(c, d_dst, fd, file_off, nbytes);
}

template <class T>
static T *host_alloc(size_t count) {
  T *p = (T *)malloc((count ? count : 1) * sizeof(T));
  if (!p) throw Error(PFP_ENOMEM, "host malloc failed");
  return p;
}
// device bytes -> a fresh host array the caller frees (free / pfp_free)
uint8_t *fetch_bytes(pfp_ctx *c, const uint8_t *d_src, uint64_t nbytes);
// a whole file into a device buffer of the pool; returns its size.  alloc_bytes(size): what to allocate for it (default: 16 bytes
// more than the file holds) - called before anything is allocated, so it may refuse the size by throwing
uint64_t file_to_dev(pfp_ctx *c, const std::string &path, DBuf<uint8_t> &d, uint64_t (*alloc_bytes)(uint64_t) = nullptr);
// device bytes -> file (created / truncated), streamed through the pinned buffers
void write_dev_file(pfp_ctx *c, const std::string &path, uint64_t file_offset, const uint8_t *d_src, uint64_t nbytes, bool trunc);
void join_background(pfp_ctx *c);      // host work that outlived a file call (MappedOut::finish)
void release_pinned(pfp_ctx *c);       // pfp_ctx_destroy: the pinned buffers and their events

// An output file whose OWN pages are the target of the device -> host copy (round 4).  write_dev_file() moves every byte
// twice on the host side of PCIe - copy engine -> pinned buffer, pwrite() -> the file's pages - and a file takes one writer at a
// time: ~6 GB/s into /dev/shm, 2.2 of the 3.5 s of the 12.6 GB command-line run.  The .bwt's size is known before the text is
// read, so: create the file at its final size, map it, and - on helper threads, beside the text input and the chain - fault
// its pages in and register the mapping with the runtime piece by piece; when the BWT exists it crosses PCIe once, at the copy
// engine's rate, straight into the file (tools/microbench/regout.hip: 31 GB/s into a populated, registered mapping against
// 4.1-4.7 for the pinned-buffer path).  Files in a memory file system only (anything else: the pwrite path); every failure on
// the way - no mapping, a piece the runtime will not register - falls back to the pwrite path for the whole file.
struct MappedOut {
  uint64_t kPiece = 128ull << 20;      // (a small file in smaller pieces: its first copy starts sooner)
  std::string path;
  int fd = -1, device = 0;
  uint8_t *m = nullptr;
  uint64_t bytes = 0, npieces = 0;
  std::vector<int> state;                 // per piece: 0 pending, 1 registered, -1 failed (under mu)
  std::mutex mu;
  std::condition_variable cv;
  std::atomic<bool> cancel{false};
  std::vector<std::thread> workers;
  hipStream_t cs = nullptr;               // the copies' own stream: the run sampling that follows the BWT overlaps them
  hipEvent_t ev = nullptr;
  bool copying = false, done = false;
  std::chrono::steady_clock::time_point t_start;
  double s_populate = 0, s_register = 0, s_ready = 0, s_waited = 0;      // PFP_TRACE_HOST (under mu)

  static bool wanted(uint64_t nbytes) {
    static const int mode = []() { const char *e = getenv("PFP_MAP_OUTPUT"); return e ? atoi(e) : -1; }();      // 0: never
    static const uint64_t min_bytes = []() { const char *e = getenv("PFP_MAP_MIN_BYTES"); return e ? (uint64_t)atoll(e) : (64ull << 20); }();      // (tests: small files too)
    return mode != 0 && nbytes >= std::max<uint64_t>(min_bytes, 1);
  }
  // false: this file is written the ordinary way
  bool start(pfp_ctx *c, const std::string &path_, uint64_t nbytes) {
    if (!wanted(nbytes)) return false;
    path = path_; bytes = nbytes; device = c->device;
    // (a disk file system tracks dirty pages through write faults, which a copy engine does not take: pwrite there)
    struct statfs sf;
    const size_t slash = path.rfind('/');
    const std::string dir = slash == std::string::npos ? std::string(".") : (slash == 0 ? std::string("/") : path.substr(0, slash));
    if (statfs(dir.c_str(), &sf) != 0 || (unsigned long)sf.f_type != 0x01021994ul /* tmpfs */) return false;
    fd = open(path.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644);
    if (fd < 0) return false;      // (the ordinary path reports it)
    if (fstatfs(fd, &sf) != 0 || (unsigned long)sf.f_type != 0x01021994ul || ftruncate(fd, (off_t)bytes) != 0) { close(fd); fd = -1; unlink(path.c_str()); return false; }
    t_start = std::chrono::steady_clock::now();
    void *q = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_SHARED, fd, 0);
    if (q == MAP_FAILED) { close(fd); fd = -1; unlink(path.c_str()); return false; }
    m = (uint8_t *)q;
    static const uint64_t piece_mb = []() { const char *e = getenv("PFP_MAP_PIECE_MB"); return e ? (uint64_t)atoll(e) : (uint64_t)32; }();
    kPiece = std::min<uint64_t>(std::max<uint64_t>(piece_mb, 2) << 20, std::max<uint64_t>(2ull << 20, (bytes / 8 + (2u << 20) - 1) & ~uint64_t((2u << 20) - 1)));
    npieces = (bytes + kPiece - 1) / kPiece;
    state.assign(npieces, 0);
    if (hipStreamCreateWithFlags(&cs, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
      (void)hipGetLastError(); abandon(true); return false;
    }
    workers.emplace_back([this]() { work(); });
    return true;
  }
  // ONE helper: page allocation in one file does not scale over threads - 1.96 s for 12.6 GB from one thread, 3.0-3.2 s from
  // 4-16, and an allocating thread beside a mapping one slows both (tools/microbench/regout.hip, profiles/r04_regout_*.txt).
  // Per piece: its pages allocated by fallocate (19 GB/s; 6 when the registration's faults have to allocate them), then
  // mapped and pinned by the registration.  Pieces of 32 MB: a registration in flight holds up the calling thread's own
  // allocations and copies (text in 0.35 -> 0.9 s, cold chain 0.6 -> 0.9 s with 128 MB pieces), smaller ones cost the helper more.
  void work() {
    (void)hipSetDevice(device);
    for (uint64_t i = 0; i < npieces && !cancel.load(); i++) {
      const uint64_t off = i * kPiece, len = std::min(kPiece, bytes - off);
      const auto a0 = std::chrono::steady_clock::now();
      // (a file system without room: no page of the piece may be touched through the mapping - that would be a SIGBUS where
      //  write() says ENOSPC; the piece counts as refused and the pwrite path reports the error)
      const bool have_pages = fallocate(fd, 0, (off_t)off, (off_t)len) == 0;
      const auto a1 = std::chrono::steady_clock::now();
      static const long fail_at = []() { const char *t = getenv("PFP_TEST_MAP_FAIL"); return t ? atol(t) : -1L; }();      // (test hook: piece k is refused)
      const hipError_t e = (long)i == fail_at || !have_pages ? hipErrorOutOfMemory : hipHostRegister(m + off, len, hipHostRegisterDefault);
      if (e != hipSuccess) (void)hipGetLastError();
      const auto a2 = std::chrono::steady_clock::now();
      {
        std::lock_guard<std::mutex> g(mu);
        state[i] = e == hipSuccess ? 1 : -1;
        s_populate += std::chrono::duration<double>(a1 - a0).count(); s_register += std::chrono::duration<double>(a2 - a1).count();
        s_ready = std::chrono::duration<double>(a2 - t_start).count();
      }
      cv.notify_all();
      if (e != hipSuccess) return;      // (the copy gives up at this piece)
    }
  }
  // device bytes [0, nbytes) -> the file, behind what the context's stream holds; returns at once (finish() waits).
  // false: a piece could not be registered - nothing usable was written, the caller takes the ordinary path.
  bool write(pfp_ctx *c, const uint8_t *d_src, uint64_t nbytes) {
    PFP_REQUIRE(nbytes <= bytes, PFP_EINVAL, "mapped output smaller than the result");
    PFP_HIP(hipEventRecord(ev, c->stream));
    PFP_HIP(hipStreamWaitEvent(cs, ev, 0));
    copying = true;
    for (uint64_t i = 0; i < npieces && i * kPiece < nbytes; i++) {
      {
        const auto a0 = std::chrono::steady_clock::now();
        std::unique_lock<std::mutex> g(mu); cv.wait(g, [&]() { return state[i] != 0; });
        s_waited += std::chrono::duration<double>(std::chrono::steady_clock::now() - a0).count();
        if (state[i] < 0) return false;
      }
      const uint64_t off = i * kPiece, len = std::min(kPiece, nbytes - off);
      PFP_HIP(hipMemcpyAsync(m + off, d_src + off, len, hipMemcpyDeviceToHost, cs));
    }
    return true;
  }
  void join_workers() { cancel.store(true); for (auto &t : workers) if (t.joinable()) t.join(); workers.clear(); }
  void unregister_all() {
    join_workers();
    if (m) for (uint64_t i = 0; i < npieces; i++) if (state[i] == 1) { (void)hipHostUnregister(m + i * kPiece); state[i] = 0; }
    if (ev) { (void)hipEventDestroy(ev); ev = nullptr; }
    if (cs) { (void)hipStreamDestroy(cs); cs = nullptr; }
  }
  // waits for the copies, gives the file its final length and lets go of the mapping.  Taking 12.6 GB out of the page table
  // costs a quarter of a second: on a thread the context joins later - the file is complete before that.  (Measured and
  // dropped: unmapping every piece as soon as its copy has landed - the address space's lock, taken for every piece, held up
  // this thread's own mappings and stream calls: files out 45 -> 125 ms at 0.79 GB.)
  void finish(pfp_ctx *c, uint64_t final_bytes) {
    const auto a0 = std::chrono::steady_clock::now();
    if (copying) PFP_HIP(hipStreamSynchronize(cs));
    copying = false;
    const auto a1 = std::chrono::steady_clock::now();
    unregister_all();
    bool ok = final_bytes == bytes || ftruncate(fd, (off_t)final_bytes) == 0;
    ok = (close(fd) == 0) && ok; fd = -1;
    done = true;
    if (getenv("PFP_TRACE_HOST"))
      fprintf(stderr, "[pfp] %s, %.2f GB through its mapping: pages allocated %.3f s, mapped and registered %.3f s (%zu pieces), all ready %.3f s after the start; the copy waited %.3f s for pieces, %.3f s for the copy engine, %.3f s to unregister and close\n",
              path.c_str(), bytes / 1e9, s_populate, s_register, (size_t)npieces, s_ready, s_waited, std::chrono::duration<double>(a1 - a0).count(),
              std::chrono::duration<double>(std::chrono::steady_clock::now() - a1).count());
    uint8_t *mm = m; const uint64_t len = bytes; m = nullptr;
    // (last: an unmapping in flight holds the address space's lock, and creating a thread or destroying a stream would wait for it)
    c->background.emplace_back([mm, len]() { munmap(mm, len); });
    PFP_REQUIRE(ok, PFP_EINVAL, "error writing " + path + ": " + strerror(errno));
  }
  // drop everything; the (incomplete) file goes too unless the ordinary path is about to rewrite it
  void abandon(bool remove) {
    if (copying && cs) (void)hipStreamSynchronize(cs);
    copying = false;
    unregister_all();
    if (m) { munmap(m, bytes); m = nullptr; }
    if (fd >= 0) { close(fd); fd = -1; if (remove) unlink(path.c_str()); }
    (void)hipGetLastError();
    done = true;
  }
  bool active() const { return m != nullptr && !done; }
  ~MappedOut() { if (!done && (m || fd >= 0)) abandon(true); }
};

}  // namespace pfp
