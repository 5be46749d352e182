// sfm_runtime.hip — what every other translation unit of libsfm_hip.so links against: the library context, the
// error text, stream_sync and the three-mode device-memory pool (declared in sfm_common.h), with the C-ABI functions
// that belong to them.  No kernels live here.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "sfm_common.h"

namespace sfm {

// ---------------------------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------------------------
static thread_local char g_err[512] = "";

Context& ctx() {
  static Context c;
  return c;
}

void set_error(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

int hip_fail(hipError_t e, const char* what, int line) {
  set_error("HIP error '%s' in %s (line %d)", hipGetErrorString(e), what, line);
  return SFM_E_HIP;
}

PendingWork& pending_work() {
  static thread_local PendingWork w;
  return w;
}

int stream_sync(hipStream_t s) {
  SFM_HIP(hipStreamSynchronize(s));
  PendingWork& w = pending_work();
  if (w.stream == s || w.stream == nullptr) w.dirty = false;
  return SFM_OK;
}

int& ba_live_problems() {
  static int n = 0;
  return n;
}

int ensure_init() {
  if (ctx().inited) return SFM_OK;
  return sfm_init(0);
}

// ---------------------------------------------------------------------------------------------
// device-memory pool (see sfm_common.h)
//
// Three process-wide modes, chosen by the environment at first use:
//   default            blocks rounded up to a power of two, cached per size class.  NO slack behind a buffer: a read past
//                      the end is not made harmless by construction (SFM_POOL_SLACK=<bytes> adds that many bytes behind
//                      every block -- a field switch for a suspected stray read, never set by the tests).
//   SFM_POOL_REDZONE=1 every buffer between two 4 KB zones of 0xA5, checked when it returns to the pool: an out-of-bounds
//                      WRITE aborts with a message.
//   SFM_POOL_GUARD=1   every buffer is its own virtual-memory mapping (hipMemAddressReserve / hipMemCreate / hipMemMap)
//                      that ENDS (to 16 bytes) where the buffer ends, followed by a reserved, never mapped granule: an
//                      out-of-bounds READ or write past the end faults at the access instead of landing in a neighbour.
//                      No caching (every free unmaps).  For one test pass on the GPU box.
// ---------------------------------------------------------------------------------------------
namespace {
struct Block { void* base; size_t size; size_t bytes; hipMemGenericAllocationHandle_t handle; size_t mapped; };
struct Pool {
  std::mutex mu;
  std::unordered_map<void*, Block> live;                  // pointer handed out -> its block
  std::unordered_map<size_t, std::vector<void*>> free_by_size;   // rounded size -> cached block bases
  size_t cached_bytes = 0;
  long long guard_allocs = 0;
  size_t guard_reserved = 0;      // address space guard mode has reserved (never returned)
};
Pool& pool() {
  static Pool p;
  return p;
}
size_t round_up_pow2(size_t n) {
  size_t r = 256;
  while (r < n) r <<= 1;
  return r;
}
constexpr size_t kPoolCap = (size_t)2 << 30;
constexpr size_t kRedZone = 4096;
bool env_is_one(const char* name) {
  const char* e = std::getenv(name);
  return e && e[0] == '1';
}
bool redzone_on() {
  static const bool on = env_is_one("SFM_POOL_REDZONE");
  return on;
}
bool guard_on() {
  static const bool on = env_is_one("SFM_POOL_GUARD");
  return on;
}
size_t slack_bytes() {
  static const size_t n = [] { const char* e = std::getenv("SFM_POOL_SLACK"); return e ? (size_t)std::strtoull(e, nullptr, 10) : (size_t)0; }();
  return n;
}
void redzone_fill(const Block& b, void* user) {
  char* base = static_cast<char*>(b.base);
  char* end = static_cast<char*>(user) + b.bytes;
  (void)hipMemset(base, 0xA5, kRedZone);
  (void)hipMemset(end, 0xA5, (size_t)(base + b.size - end));
}
void redzone_check(const Block& b, void* user) {
  (void)hipDeviceSynchronize();
  char* base = static_cast<char*>(b.base);
  char* end = static_cast<char*>(user) + b.bytes;
  const size_t tail = (size_t)(base + b.size - end);
  std::vector<unsigned char> h(std::max(kRedZone, tail));
  auto scan = [&](const char* what, const char* dev, size_t n) {
    (void)hipMemcpy(h.data(), dev, n, hipMemcpyDeviceToHost);
    for (size_t i = 0; i < n; ++i)
      if (h[i] != 0xA5) {
        std::fprintf(stderr, "sfm pool red zone: a kernel wrote %s a %zu-byte buffer (offset %zu of the zone)\n", what, b.bytes, i);
        std::abort();
      }
  };
  scan("BEFORE", base, kRedZone);
  scan("PAST THE END OF", end, tail);
}

// ---- guard mode --------------------------------------------------------------------------------
size_t guard_granularity(int device) {
  static size_t g = 0;
  if (g) return g;
  hipMemAllocationProp prop{};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = device;
  size_t gran = 0;
  if (hipMemGetAllocationGranularity(&gran, &prop, hipMemAllocationGranularityMinimum) != hipSuccess || gran == 0) gran = (size_t)2 << 20;
  g = gran;
  return g;
}
hipError_t guard_alloc(void** ptr, size_t bytes, Block* out) {
  const int device = ctx().device < 0 ? 0 : ctx().device;
  const size_t gran = guard_granularity(device);
  const size_t need = (std::max<size_t>(bytes, 1) + 15) & ~(size_t)15;      // vector loads are at most 16 bytes wide
  const size_t mapped = (need + gran - 1) / gran * gran;
  void* base = nullptr;
  hipError_t e = hipMemAddressReserve(&base, mapped + gran, gran, nullptr, 0);      // + one granule that is never mapped
  if (e != hipSuccess) return e;
  hipMemAllocationProp prop{};
  prop.type = hipMemAllocationTypePinned;
  prop.location.type = hipMemLocationTypeDevice;
  prop.location.id = device;
  hipMemGenericAllocationHandle_t h{};
  e = hipMemCreate(&h, mapped, &prop, 0);
  if (e != hipSuccess) { (void)hipMemAddressFree(base, mapped + gran); return e; }
  e = hipMemMap(base, mapped, 0, h, 0);
  if (e != hipSuccess) { (void)hipMemRelease(h); (void)hipMemAddressFree(base, mapped + gran); return e; }
  hipMemAccessDesc acc{};
  acc.location.type = hipMemLocationTypeDevice;
  acc.location.id = device;
  acc.flags = hipMemAccessFlagsProtReadWrite;
  e = hipMemSetAccess(base, mapped, &acc, 1);
  if (e != hipSuccess) { (void)hipMemUnmap(base, mapped); (void)hipMemRelease(h); (void)hipMemAddressFree(base, mapped + gran); return e; }
  *ptr = static_cast<char*>(base) + (mapped - need);      // the buffer ends where the mapping ends
  *out = Block{base, mapped + gran, bytes, h, mapped};
  return hipSuccess;
}
void guard_free(const Block& b) {
  (void)hipDeviceSynchronize();
  (void)hipMemUnmap(b.base, b.mapped);
  (void)hipMemRelease(b.handle);
  // The address range stays RESERVED for the life of the process: hipMemAddressFree followed by a new reservation hands
  // the same addresses out again, and on this stack (ROCm 7.2, MI355X) the device then kept reading through stale
  // translations -- 85 of 200 upload / kernel / download round trips came back wrong and BA results varied from run to run
  // (profiles/r3/guard_mode_diagnostic.txt); with every range used once the same runs are exact.  A never-reused range also
  // turns a use-after-free into a fault.  The suite reserves a few hundred GB of the 47-bit address space this way.
}
}  // namespace

hipError_t pool_alloc(void** ptr, size_t bytes) {
  Pool& P = pool();
  if (bytes > ((size_t)1 << 40)) return hipErrorOutOfMemory;      // a size computed from a negative count: fail, do not loop in round_up_pow2
  if (guard_on()) {
    // guard mode never hands an address range out twice (guard_free), i.e. it leaks address space by design: it is a TEST
    // mode.  A long-lived process must not run into the end of the 47-bit space unannounced: stop at 16 TB.
    if (P.guard_reserved + bytes > ((size_t)16 << 40)) {
      std::fprintf(stderr, "sfm pool guard mode: %zu GB of address space reserved and never reused; SFM_POOL_GUARD is a test mode, not for long-lived processes\n",
                   P.guard_reserved >> 30);
      std::abort();
    }
    P.guard_reserved += bytes + (64 << 10);
    Block b{};
    const hipError_t e = guard_alloc(ptr, bytes, &b);
    if (e != hipSuccess) {
      std::fprintf(stderr, "sfm pool guard mode: the virtual-memory API failed (%s); SFM_POOL_GUARD cannot be honoured on this stack\n", hipGetErrorString(e));
      std::abort();      // a test pass that silently ran unguarded would claim what it did not check
    }
    std::lock_guard<std::mutex> g(P.mu);
    P.live[*ptr] = b;
    ++P.guard_allocs;
    return hipSuccess;
  }
  const bool rz = redzone_on();
  // size class = the request rounded up to a power of two up to 64 MB, to the next multiple of 2 MB above (VERDICT r3 item 8:
  // the 169 MB Zd of C3 took a 256 MB class, 3.7 GB of C4 took 4 GB; large buffers are few and long-lived, so a fine class
  // costs no reuse); red zones / optional slack come on top of the class, so a request that already is a class size does
  // not grow
  constexpr size_t kFineAbove = (size_t)64 << 20, kFineStep = (size_t)2 << 20;
  const size_t cls = bytes <= kFineAbove ? round_up_pow2(bytes) : (bytes + kFineStep - 1) / kFineStep * kFineStep;
  const size_t sz = cls + (rz ? 2 * kRedZone : slack_bytes());
  void* base = nullptr;
  {
    std::lock_guard<std::mutex> g(P.mu);
    auto it = P.free_by_size.find(sz);
    if (it != P.free_by_size.end() && !it->second.empty()) {
      base = it->second.back();
      it->second.pop_back();
      P.cached_bytes -= sz;
    }
  }
  if (base == nullptr) {
    hipError_t e = hipMalloc(&base, sz);
    if (e != hipSuccess) {               // out of memory: drop the cache and retry once
      pool_release_all();
      e = hipMalloc(&base, sz);
    }
    if (e != hipSuccess) return e;
  }
  *ptr = rz ? static_cast<char*>(base) + kRedZone : base;
  const Block b{base, sz, bytes, {}, 0};
  if (rz) redzone_fill(b, *ptr);
  std::lock_guard<std::mutex> g(P.mu);
  P.live[*ptr] = b;
  return hipSuccess;
}

void pool_free(void* ptr) {
  if (ptr == nullptr) return;
  Pool& P = pool();
  Block b{};
  {
    std::lock_guard<std::mutex> g(P.mu);
    auto it = P.live.find(ptr);
    if (it == P.live.end()) { (void)hipFree(ptr); return; }     // not ours (defensive)
    b = it->second;
    P.live.erase(it);
  }
  if (b.mapped) { guard_free(b); return; }
  if (redzone_on()) redzone_check(b, ptr);
  {
    std::lock_guard<std::mutex> g(P.mu);
    if (P.cached_bytes + b.size <= kPoolCap) {
      P.free_by_size[b.size].push_back(b.base);
      P.cached_bytes += b.size;
      return;
    }
  }
  (void)hipFree(b.base);
}

void pool_release_all() {
  Pool& P = pool();
  std::lock_guard<std::mutex> g(P.mu);
  for (auto& kv : P.free_by_size)
    for (void* q : kv.second) (void)hipFree(q);
  P.free_by_size.clear();
  P.cached_bytes = 0;
}

// Diagnostics of the pool mode (sfm_pool_mode): bit 0 red zones, bit 1 guard mappings; *tail_slack = bytes between the
// end of a probe buffer of `probe_bytes` and the end of what is mapped behind it (guard mode: < 16).
int pool_mode_probe(size_t probe_bytes, long long* tail_slack, long long* guard_allocs) {
  int mode = (redzone_on() ? 1 : 0) | (guard_on() ? 2 : 0);
  if (tail_slack) {
    *tail_slack = -1;
    if (ctx().inited) {
      void* q = nullptr;
      if (pool_alloc(&q, probe_bytes) == hipSuccess) {
        Pool& P = pool();
        {
          std::lock_guard<std::mutex> g(P.mu);
          const Block& b = P.live[q];
          const char* end_mapped = static_cast<char*>(b.base) + (b.mapped ? b.mapped : b.size);
          *tail_slack = (long long)(end_mapped - (static_cast<char*>(q) + probe_bytes));
        }
        pool_free(q);
      }
    }
  }
  if (guard_allocs) *guard_allocs = pool().guard_allocs;
  return mode;
}

}  // namespace sfm

using namespace sfm;

extern "C" {

int sfm_version(void) { return 112; }

const char* sfm_last_error(void) { return g_err; }

int sfm_init(int device) {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count <= 0) {
    set_error("no HIP device visible (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
    return SFM_E_NO_DEVICE;
  }
  if (device < 0 || device >= count) {
    set_error("device %d out of range (0..%d)", device, count - 1);
    return SFM_E_NO_DEVICE;
  }
  Context& c = ctx();
  if (c.inited && c.device == device) return SFM_OK;
  if (c.inited) sfm_shutdown();
  SFM_HIP(hipSetDevice(device));
  hipDeviceProp_t prop;
  SFM_HIP(hipGetDeviceProperties(&prop, device));
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
    set_error("device %d is %s; this library ships gfx950 (MI355X) code objects only", device, prop.gcnArchName);
    return SFM_E_NO_DEVICE;
  }
  c.num_cus = prop.multiProcessorCount;
  SFM_HIP(hipStreamCreateWithFlags(&c.own, hipStreamNonBlocking));
  c.stream = c.own;
  c.device = device;
  c.inited = true;
  return SFM_OK;
}

int sfm_shutdown(void) {
  Context& c = ctx();
  if (!c.inited) return SFM_OK;
  (void)hipStreamSynchronize(c.stream);
  if (c.stream != c.own) (void)hipStreamSynchronize(c.own);
  (void)hipDeviceSynchronize();      // the split-PnP workspaces belong to callers' streams
  pnp_split_release();
  pool_release_all();
  if (c.own) (void)hipStreamDestroy(c.own);
  const int cu_limit = c.cu_limit;      // the test hook outlives the device (it works before sfm_init)
  c = Context();
  c.cu_limit = cu_limit;
  return SFM_OK;
}

int sfm_set_cu_limit(int n) {
  if (n < 0) { set_error("sfm_set_cu_limit: n = %d is negative (0 removes the limit)", n); return SFM_E_SHAPE; }
  if (ba_live_problems() > 0) {
    set_error("sfm_set_cu_limit: %d sfm_ba_problem handle(s) exist, and their workspaces were sized for the current count; destroy them first",
              ba_live_problems());
    return SFM_E_SHAPE;
  }
  ctx().cu_limit = n;
  return SFM_OK;
}

int sfm_cu_count(int* device, int* effective) {
  if (device) *device = ctx().num_cus;
  if (effective) *effective = plan_cus();
  return SFM_OK;
}

int sfm_set_stream(void* hip_stream) {
  SFM_TRY(ensure_init());
  Context& c = ctx();
  // the library's own stream lives from sfm_init to sfm_shutdown, so a problem that captured it as its default
  // (sfm_ba_create) never holds a dangling handle; an installed stream stays the caller's
  SFM_HIP(hipStreamSynchronize(c.stream));
  c.stream = hip_stream == nullptr ? c.own : reinterpret_cast<hipStream_t>(hip_stream);
  return SFM_OK;
}

int sfm_synchronize(void) {
  SFM_TRY(ensure_init());
  SFM_TRY(stream_sync(ctx().stream));
  return SFM_OK;
}

int sfm_pool_redzone_active(void) { return redzone_on() ? 1 : 0; }

int sfm_pool_mode(int64_t probe_bytes, int64_t* tail_slack, int64_t* guard_allocs) {
  long long slack = -1, allocs = 0;
  const int mode = pool_mode_probe(probe_bytes > 0 ? (size_t)probe_bytes : 1, tail_slack ? &slack : nullptr, &allocs);
  if (tail_slack) *tail_slack = slack;
  if (guard_allocs) *guard_allocs = allocs;
  return mode;
}

}  // extern "C"
