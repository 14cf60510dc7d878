// api_ctx.hip -- the context's life and settings (include/pfpgpu.h): version, errors, create / destroy, switches, statistics,
// kernel trace, the device pool's calls, and the frees and the copy for buffers the library handed out.
#include "api.hpp"

using namespace pfp;

extern "C" {

const char *pfp_version(void) { return "pfpgpu 0.1 (gfx950, wave64; prefix-free parsing BWT)"; }

const char *pfp_strerror(int code) {
  switch (code) {
    case PFP_OK: return "ok";
    case PFP_EINVAL: return "invalid argument";
    case PFP_ENODEV: return "no usable HIP device";
    case PFP_EHIP: return "HIP runtime error";
    case PFP_ECOLLISION: return "phrase hash collision";
    case PFP_ELIMIT: return "size limit exceeded";
    case PFP_EFORMAT: return "inconsistent input";
    case PFP_ENOMEM: return "out of memory";
    case PFP_ESHORT: return "input too short";
    default: return "unknown error";
  }
}

int pfp_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
  return n;
}
int pfp_ctx_create(pfp_ctx **out, int device) {
  if (!out) return PFP_EINVAL;
  *out = nullptr;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || device < 0 || device >= ndev) {
    (void)hipGetLastError();
    return PFP_ENODEV;
  }
  pfp_ctx *c = new (std::nothrow) pfp_ctx();
  if (!c) return PFP_ENOMEM;
  try {
    c->device = device;
    PFP_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    PFP_HIP(hipGetDeviceProperties(&prop, device));
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    PFP_HIP(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->pool.stream = c->stream;
    { const char *pd = getenv("PFP_POOL_DEBUG"); c->pool.debug = pd && pd[0] && pd[0] != '0'; }
    { const char *tl = getenv("PFP_TEST_POOL_LIMIT"); if (tl) c->pool.test_limit = (size_t)strtoull(tl, nullptr, 10); }
    c->pool.trace = getenv("PFP_TRACE_POOL") != nullptr;
    { size_t fr = 0, tot = 0; if (hipMemGetInfo(&fr, &tot) == hipSuccess) c->pool.soft_limit = tot / 10 * 7; else (void)hipGetLastError(); }
    PFP_HIP(hipHostMalloc((void **)&c->h_scalars, 16 * sizeof(uint64_t), hipHostMallocDefault));
    const char *dbg = getenv("PFP_DEBUG");
    c->debug = dbg && dbg[0] && dbg[0] != '0';
    { const char *fw = getenv("PFP_FORCE_IDX64"); c->force_wide = fw && fw[0] && fw[0] != '0'; }
    { const char *wh = getenv("PFP_WINDOW_HASH"); if (wh && !strcmp(wh, "kr")) c->fast_triggers = false; }
    { const char *pd = getenv("PFP_PARSE_DENSITY"); if (pd && atof(pd) >= 0.01 && atof(pd) <= 64.0) c->parse_density = atof(pd); }
    (void)hipGetLastError();
  } catch (const pfp::Error &e) {
    (void)hipGetLastError();
    delete c;
    return e.code == PFP_EHIP ? PFP_ENODEV : e.code;
  }
  *out = c;
  return PFP_OK;
}

void pfp_ctx_destroy(pfp_ctx *c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  join_background(c);
  pfp_dist_release(c);
  release_debug_state(c);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  c->kt.destroy();
  if (getenv("PFP_TRACE_HOST")) fprintf(stderr, "[pfp] host waits on the stream over the context's life: %llu\n", (unsigned long long)c->n_syncs);
  c->pool.print_peak();
  c->pool.destroy();
  if (c->h_scalars) (void)hipHostFree(c->h_scalars);
  release_pinned(c);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

const char *pfp_last_error(const pfp_ctx *c) { return c ? c->err.c_str() : "null context"; }
int pfp_debug_check(pfp_ctx *c) {
  if (!c) return PFP_EINVAL;
  if (c->pool.corrupt.empty()) return PFP_OK;
  c->err = c->pool.corrupt;
  return PFP_EHIP;
}
void pfp_pool_trim(pfp_ctx *c) {      // give the cached device blocks back to the driver (several contexts sharing one GPU)
  if (!c) return;
  (void)hipSetDevice(c->device);
  c->pool.trim();
}
int pfp_get_mem_stats(const pfp_ctx *c, uint64_t out[4]) {
  if (!c || !out) return PFP_EINVAL;
  out[0] = c->pool.total_bytes; out[1] = c->pool.peak_bytes; out[2] = c->pool.live_bytes; out[3] = c->pool.debug ? c->pool.debug_blocks : 0;
  return PFP_OK;
}
int pfp_get_pool_counters(const pfp_ctx *c, uint64_t out[2]) {
  if (!c || !out) return PFP_EINVAL;
  out[0] = c->pool.driver_allocs; out[1] = c->pool.trims;
  return PFP_OK;
}
void *pfp_ctx_stream(pfp_ctx *c) { return c ? (void *)c->stream : nullptr; }
void pfp_free(void *p) { free(p); }
void pfp_set_profiling(pfp_ctx *c, int on) { if (c) c->profiling = on != 0; }
void pfp_set_kernel_trace(pfp_ctx *c, int on) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  c->kt.resolve();
  c->kt.agg.clear();
  c->kt.on = on != 0;
}
int pfp_get_kernel_trace(pfp_ctx *c, pfp_kernel_stat *out, int cap) {
  if (!c) return PFP_EINVAL;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  c->kt.resolve();
  int k = 0;
  for (auto &kv : c->kt.agg) {
    if (out && k < cap) {
      memset(&out[k], 0, sizeof out[k]);
      strncpy(out[k].name, kv.first.c_str(), sizeof out[k].name - 1);
      out[k].launches = kv.second.launches; out[k].total_ms = kv.second.ms; out[k].algo_bytes = kv.second.bytes;
    }
    k++;
  }
  return k;
}
void pfp_set_max_phrase(pfp_ctx *c, uint64_t max_phrase) { if (c) c->max_phrase = max_phrase; }
void pfp_set_window_hash(pfp_ctx *c, int fast) { if (c) c->fast_triggers = fast != 0; }
int pfp_set_parse_density(pfp_ctx *c, double density) {
  if (!c || !(density == 0.0 || (density >= 0.01 && density <= 64.0))) return PFP_EINVAL;
  c->parse_density = density;
  return PFP_OK;
}
int pfp_set_index_bits(pfp_ctx *c, int bits) {
  if (!c || (bits != 0 && bits != 32 && bits != 64)) return PFP_EINVAL;
  c->force_wide = bits == 64;
  c->force_narrow = bits == 32;
  return PFP_OK;
}
int pfp_get_stats(const pfp_ctx *c, pfp_stats *st) {
  if (!c || !st) return PFP_EINVAL;
  *st = c->stats;
  return PFP_OK;
}

void pfp_parse_result_free(pfp_parse_result *r) {
  if (!r) return;
  free(r->dict); free(r->occ); free(r->parse); free(r->last); free(r->sai);
  memset(r, 0, sizeof *r);
}
void pfp_bwt_result_free(pfp_bwt_result *r) {
  if (!r) return;
  free(r->bwt); free(r->sa); free(r->ssa); free(r->esa);
  memset(r, 0, sizeof *r);
}

int pfp_memcpy_d2h(pfp_ctx *c, void *host_dst, const void *d_src, uint64_t nbytes) {
  if (!c || ((!host_dst || !d_src) && nbytes)) return PFP_EINVAL;
  PFP_TRY_DEV(c)
  download(c, host_dst, (const uint8_t *)d_src, nbytes);
  sync(c);
  return PFP_OK;
  PFP_CATCH(c)
}
void pfp_dev_free(pfp_ctx *c, void *d_ptr) {
  if (!c || !d_ptr) return;
  (void)hipSetDevice(c->device);
  for (const auto &b : c->pool.all)
    if (b.p == d_ptr) { c->pool.put(d_ptr); return; }      // (later work of the context is ordered behind the caller's reads only if
  (void)hipFree(d_ptr);                                    //  those were on the context's stream or have completed: pfpgpu.h)
}

}  // extern "C"
