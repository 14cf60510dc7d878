// hostio.hip -- host memory and files <-> HBM: every byte crosses in chunks through the context's two pinned buffers (the only
// code that touches them), double-buffered against the copy engine; text staging; whole files in and out.
#include "hostio.hpp"
#include <cerrno>
#include <sys/stat.h>

namespace pfp {

// work(offset, length) over [0, len) cut into at most T parts of whole 4 KiB pages, a thread per part (T <= 1: the caller's)
template <class Work>
static void split_range(size_t len, size_t T, Work &&work) {
  if (T <= 1) { work(size_t(0), len); return; }
  const size_t part = ((len + T - 1) / T + 4095) & ~size_t(4095);
  std::vector<std::thread> th;
  for (size_t k = 0; k < T && k * part < len; k++) th.emplace_back([&work, k, part, len]() { work(k * part, std::min(part, len - k * part)); });
  for (auto &t : th) t.join();
}
static size_t host_threads(size_t wanted) {
  const unsigned hw = std::thread::hardware_concurrency();
  return std::min<size_t>(wanted, hw ? hw : 1);
}

// host-side copy with a few threads: one core moves ~10 GB/s, PCIe Gen5 x16 takes 50
static void par_memcpy(void *dst, const void *src, size_t len) {
  split_range(len, std::min<size_t>(host_threads(8), len >> 22),
              [=](size_t off, size_t l) { memcpy((uint8_t *)dst + off, (const uint8_t *)src + off, l); });
}

// the same from a file: a few threads pread their parts straight into the (pinned) destination - one copy out of the page
// cache and no page-table work, where an mmap'ed source costs a fault per 4 KB page (12.6 GB in /dev/shm: 2 GB/s through the
// mapping, an order of magnitude more through pread)
static void par_pread(int fd, uint64_t file_off, void *dst, size_t len) {
  static const size_t tmax = []() { const char *e = getenv("PFP_READ_THREADS"); return e ? (size_t)atoi(e) : (size_t)8; }();
  std::atomic<int> bad{0};
  split_range(len, std::min<size_t>(host_threads(tmax), len >> 21), [&](size_t off, size_t l) {
    size_t done = 0;
    while (done < l) {
      const ssize_t r = pread(fd, (uint8_t *)dst + off + done, l - done, (off_t)(file_off + off + done));
      if (r <= 0) { bad.store(r == 0 ? -1 : errno ? errno : -1); return; }
      done += (size_t)r;
    }
  });
  PFP_REQUIRE(bad.load() == 0, PFP_EINVAL, bad.load() == -1 ? std::string("input file is shorter than announced") : std::string("reading the input: ") + strerror(bad.load()));
}

static void ensure_pinned(pfp_ctx *c) {
  for (int k = 0; k < 2; k++) {
    // (PFP_PIN_NONCOHERENT=1: host-cacheable staging buffers - the CPU fills them, the copy engine reads them)
    static const unsigned pin_flags = getenv("PFP_PIN_NONCOHERENT") ? hipHostMallocNonCoherent : hipHostMallocDefault;
    if (!c->pin[k]) PFP_HIP(hipHostMalloc(&c->pin[k], pfp_ctx::kPinBytes, pin_flags));
    if (!c->pin_ev[k]) PFP_HIP(hipEventCreateWithFlags(&c->pin_ev[k], hipEventDisableTiming));
  }
}
// Device -> host stream in chunks through the two pinned buffers: while chunk i crosses PCIe, `sink`
// consumes chunk i-1 on the host (file write, copy into the caller's buffer).
template <class Sink>
static void stream_d2h(pfp_ctx *c, const uint8_t *d_src, uint64_t nbytes, Sink &&sink) {
  ensure_pinned(c);
  const uint64_t CH = pfp_ctx::kPinBytes;
  uint64_t prev_off = 0, prev_len = 0;
  int k = 0;
  for (uint64_t off = 0; off < nbytes || prev_len; off += CH) {
    const uint64_t len = off < nbytes ? std::min<uint64_t>(CH, nbytes - off) : 0;
    if (len) {
      PFP_HIP(hipMemcpyAsync(c->pin[k], d_src + off, len, hipMemcpyDeviceToHost, c->stream));
      PFP_HIP(hipEventRecord(c->pin_ev[k], c->stream));
    }
    if (prev_len) {
      PFP_HIP(hipEventSynchronize(c->pin_ev[k ^ 1]));
      sink((const uint8_t *)c->pin[k ^ 1], prev_off, prev_len);
    }
    prev_off = off; prev_len = len;
    k ^= 1;
  }
}
// Host -> device the same way: `fill` writes chunk i into a pinned buffer while chunk i-1 crosses PCIe.
template <class Fill>
static void stream_h2d(pfp_ctx *c, uint8_t *d_dst, uint64_t nbytes, Fill &&fill) {
  ensure_pinned(c);
  const uint64_t CH = pfp_ctx::kPinBytes;
  static const bool trace_host = getenv("PFP_TRACE_HOST") != nullptr;
  auto now = []() { return std::chrono::steady_clock::now(); };
  auto secs = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double>(b - a).count(); };
  double t_wait = 0, t_fill = 0, t_issue = 0;
  int k = 0;
  for (uint64_t off = 0; off < nbytes; off += CH, k ^= 1) {
    const uint64_t len = std::min<uint64_t>(CH, nbytes - off);
    const auto a0 = now();
    if (off >= 2 * CH) PFP_HIP(hipEventSynchronize(c->pin_ev[k]));      // the copy that last used this buffer is done
    const auto a1 = now();
    fill((uint8_t *)c->pin[k], off, len);
    const auto a2 = now();
    PFP_HIP(hipMemcpyAsync(d_dst + off, c->pin[k], len, hipMemcpyHostToDevice, c->stream));
    PFP_HIP(hipEventRecord(c->pin_ev[k], c->stream));
    if (trace_host) { t_wait += secs(a0, a1); t_fill += secs(a1, a2); t_issue += secs(a2, now()); }
  }
  if (trace_host && nbytes >= (64u << 20))
    fprintf(stderr, "[pfp] host -> device, %.2f GB in %llu-MB pieces: filling the pinned buffers %.3f s, waiting for the copy engine %.3f s, issuing %.3f s\n",
            nbytes / 1e9, (unsigned long long)(CH >> 20), t_fill, t_wait, t_issue);
}

void upload(pfp_ctx *c, uint8_t *d_dst, const void *src, uint64_t nbytes) {
  stream_h2d(c, d_dst, nbytes, [&](uint8_t *pin, uint64_t off, uint64_t len) { par_memcpy(pin, (const uint8_t *)src + off, len); });
}
void upload_fd(pfp_ctx *c, uint8_t *d_dst, int fd, uint64_t file_off, uint64_t nbytes) {
  stream_h2d(c, d_dst, nbytes, [&](uint8_t *pin, uint64_t off, uint64_t len) { par_pread(fd, file_off + off, pin, len); });
}
void download(pfp_ctx *c, void *dst, const uint8_t *d_src, uint64_t nbytes) {
  stream_d2h(c, d_src, nbytes, [&](const uint8_t *pin, uint64_t off, uint64_t len) { par_memcpy((uint8_t *)dst + off, pin, len); });
}

// zeros and the leading Dollar in front of the text's place
static void stage_front(pfp_ctx *c, StagedText &tx, uint64_t n, int w) {
  tx.n = n; tx.w = w;
  tx.buf.alloc(c, StagedText::kFront + n + (size_t)w + StagedText::kBack);
  PFP_HIP(hipMemsetAsync(tx.buf.p, 0, StagedText::kFront - 1, c->stream));
  PFP_HIP(hipMemsetAsync(tx.buf.p + StagedText::kFront - 1, kDollar, 1, c->stream));
}
void StagedText::stage(pfp_ctx *c, const void *src, bool src_on_device, uint64_t n_, int w_) {
  stage_front(c, *this, n_, w_);
  if (n && src_on_device) PFP_HIP(hipMemcpyAsync(buf.p + kFront, src, n, hipMemcpyDeviceToDevice, c->stream));
  if (n && !src_on_device) upload(c, buf.p + kFront, src, n);      // pageable host text (a caller's buffer, an mmap of the input file)
  restage_tail(c, n, w);
}
void StagedText::stage_fd(pfp_ctx *c, int fd, uint64_t file_off, uint64_t n_, int w_) {
  stage_front(c, *this, n_, w_);
  if (n) upload_fd(c, buf.p + kFront, fd, file_off, n);
  restage_tail(c, n, w);
}
void StagedText::restage_tail(pfp_ctx *c, uint64_t new_n, int w_) const {
  PFP_HIP(hipMemsetAsync(buf.p + kFront + new_n, kDollar, (size_t)w_, c->stream));
  PFP_HIP(hipMemsetAsync(buf.p + kFront + new_n + w_, 0, kBack, c->stream));
}

// (the first touch of the fresh pages and the copy are spread over a few threads)
uint8_t *fetch_bytes(pfp_ctx *c, const uint8_t *d_src, uint64_t nbytes) {
  uint8_t *h = nullptr;
  if (nbytes >= (64u << 20)) {      // large result: 2 MiB pages where the kernel offers them (hundreds of first-touch faults, not hundreds of thousands)
    void *q = nullptr;
    if (posix_memalign(&q, 2u << 20, nbytes) == 0 && q) { (void)madvise(q, nbytes, MADV_HUGEPAGE); h = (uint8_t *)q; }
  }
  if (!h) h = host_alloc<uint8_t>(nbytes);
  try { download(c, h, d_src, nbytes); } catch (...) { free(h); throw; }
  return h;
}

void write_dev_file(pfp_ctx *c, const std::string &path, uint64_t file_offset, const uint8_t *d_src, uint64_t nbytes, bool trunc) {
  const int fd = open(path.c_str(), O_WRONLY | O_CREAT | (trunc ? O_TRUNC : 0), 0644);
  PFP_REQUIRE(fd >= 0, PFP_EINVAL, "cannot open " + path + ": " + strerror(errno));
  if (trunc && nbytes) (void)!ftruncate(fd, (off_t)(file_offset + nbytes));      // the final size at once: the writers only fill pages
  bool ok = true;
  std::string werr;
  // (round 4, measured and dropped: a shared mapping of the output file filled by eight threads - buffered pwrite()s to one file
  //  serialise on the inode - was SLOWER into /dev/shm, 2.9-3.3 s against 1.95 s for 13.7 GB: faulting fresh pages in through a
  //  mapping costs more than the write path's own allocation.  profiles/r04_cli_probe_mmap_output.txt)
  try {
    // a chunk can be written by several threads, each its own range at its own offset (PFP_PWRITE_THREADS; pfthreads.hpp:369-376
    // has every worker pwrite its range).  Default one: on tmpfs more writers only contend (1.1 GB: 172 ms with one
    // thread, 220-290 ms with 2-8, MI355X box).
    std::mutex mu;
    stream_d2h(c, d_src, nbytes, [&](const uint8_t *h, uint64_t off, uint64_t len) {
      static const unsigned wthreads = []() { const char *e = getenv("PFP_PWRITE_THREADS"); return e ? (unsigned)atoi(e) : 1u; }();
      split_range(len, std::min<size_t>(host_threads(wthreads ? wthreads : 1), std::max<size_t>(len >> 22, 1)), [&](size_t lo, size_t l) {
        size_t done = lo;
        while (done < lo + l) {
          const ssize_t w = pwrite(fd, h + done, lo + l - done, (off_t)(file_offset + off + done));
          if (w <= 0) { std::lock_guard<std::mutex> g(mu); ok = false; werr = strerror(errno); return; }
          done += (size_t)w;
        }
      });
    });
  } catch (...) { close(fd); throw; }
  sync(c);
  PFP_REQUIRE(close(fd) == 0 && ok, PFP_EINVAL, "error writing " + path + ": " + werr);
}

uint64_t file_to_dev(pfp_ctx *c, const std::string &path, DBuf<uint8_t> &d, uint64_t (*alloc_bytes)(uint64_t)) {
  const int fd = open(path.c_str(), O_RDONLY);
  struct stat sb;
  if (fd < 0 || fstat(fd, &sb) != 0) {
    if (fd >= 0) close(fd);
    throw Error(PFP_EINVAL, "cannot read " + path + ": " + strerror(errno));
  }
  const uint64_t bytes = (uint64_t)sb.st_size;
  try {
    d.alloc(c, alloc_bytes ? alloc_bytes(bytes) : bytes + 16);
    upload_fd(c, d.p, fd, 0, bytes);
    sync(c);
  } catch (...) { close(fd); throw; }
  close(fd);
  return bytes;
}

void join_background(pfp_ctx *c) {
  for (auto &t : c->background) if (t.joinable()) t.join();
  c->background.clear();
}
void release_pinned(pfp_ctx *c) {
  for (int k = 0; k < 2; k++) {
    if (c->pin[k]) (void)hipHostFree(c->pin[k]);
    if (c->pin_ev[k]) (void)hipEventDestroy(c->pin_ev[k]);
  }
}

}  // namespace pfp
