// A HIP runtime made of the host heap, for the sanitizer build of the HOST half of libpysdr_hip.so
// (tests/host_san): "device" memory is malloc'ed (so AddressSanitizer sees every size the host code
// passes to a copy or to a kernel), copies are memcpy, streams and events complete at once.  Only the
// calls the host files of pysdr_amd/csrc (api*.hip) make exist.  Nothing here is part of the product.
//   HOST_SAN_TRACE=<file>    one line per stream-ordered operation (copies, fills, event records, waits, synchronises; the
//                            launch layer adds its launches).  Streams, events and allocations are named by the order in
//                            which the TRACE first meets them (+ byte offset), never by address or creation order: allocating
//                            in another order leaves the trace as it is, using the wrong buffer of a pair does not.
//   FAKE_HIP_FAIL_ALLOC=<n>  the n-th hipMalloc / hipHostMalloc / event / stream creation of the process returns an error
//                            (fake_hip::state().fail_at: `san_main allocfail` re-arms it in process).
#pragma once
#include <chrono>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <utility>

typedef int hipError_t;
constexpr hipError_t hipSuccess = 0;
constexpr hipError_t hipErrorInvalidValue = 1;
inline const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "hipSuccess" : "fake hip error"; }
inline hipError_t hipGetLastError() { return hipSuccess; }

struct float2 { float x, y; };
struct float4 { float x, y, z, w; };
inline float2 make_float2(float x, float y) { return float2{x, y}; }
inline float4 make_float4(float x, float y, float z, float w) { return float4{x, y, z, w}; }

struct fake_stream { int id; };
struct fake_event { std::chrono::steady_clock::time_point t; bool recorded; };
typedef fake_stream* hipStream_t;
typedef fake_event* hipEvent_t;
constexpr unsigned hipStreamNonBlocking = 1, hipEventDisableTiming = 2, hipHostMallocDefault = 0;
enum hipMemcpyKind { hipMemcpyHostToHost, hipMemcpyHostToDevice, hipMemcpyDeviceToHost, hipMemcpyDeviceToDevice };

namespace fake_hip {
struct State {
  std::FILE* f = nullptr;                                       // the trace (nullptr: off, and nothing below is kept)
  std::mutex mu;
  std::map<uintptr_t, std::pair<size_t, int>> allocs;           // live allocations: base -> (bytes, trace name or -1)
  std::map<const void*, int> streams, events;
  int next_buf = 0, next_stream = 0, next_event = 0;
  long creations = 0, fail_at = 0;                              // allocation-failure injection
  bool fail_hit = false;
  State() {
    const char* p = std::getenv("HOST_SAN_TRACE");
    if (p && *p) f = std::fopen(p, "w");
    const char* q = std::getenv("FAKE_HIP_FAIL_ALLOC");
    if (q) fail_at = std::atol(q);
  }
  ~State() { if (f) std::fclose(f); }
};
inline State& state() { static State s; return s; }
inline bool tracing() { return state().f != nullptr; }
inline bool creation_fails() {
  State& s = state();
  std::lock_guard<std::mutex> lk(s.mu);
  if (++s.creations != s.fail_at) return false;
  s.fail_hit = true;
  return true;
}
inline void on_alloc(void* p, size_t n) {
  if (!tracing() || !p) return;
  std::lock_guard<std::mutex> lk(state().mu);
  state().allocs[reinterpret_cast<uintptr_t>(p)] = {n ? n : 1, -1};
}
inline void on_free(void* p) {
  if (!tracing() || !p) return;
  std::lock_guard<std::mutex> lk(state().mu);
  state().allocs.erase(reinterpret_cast<uintptr_t>(p));
}
inline std::string ptr_name(const void* p) {                    // "b<k>+<offset>" inside a live allocation, else "host"
  if (!p) return "null";
  State& s = state();
  std::lock_guard<std::mutex> lk(s.mu);
  const uintptr_t a = reinterpret_cast<uintptr_t>(p);
  auto it = s.allocs.upper_bound(a);
  if (it == s.allocs.begin()) return "host";
  --it;
  if (a - it->first >= it->second.first) return "host";
  if (it->second.second < 0) it->second.second = s.next_buf++;
  return "b" + std::to_string(it->second.second) + "+" + std::to_string(a - it->first);
}
inline std::string handle_name(std::map<const void*, int>& m, int& next, const char* prefix, const void* h) {
  if (!h) return std::string(prefix) + "-null";
  std::lock_guard<std::mutex> lk(state().mu);
  auto it = m.find(h);
  if (it == m.end()) it = m.emplace(h, next++).first;
  return prefix + std::to_string(it->second);
}
inline std::string stream_name(const void* s) { return handle_name(state().streams, state().next_stream, "s", s); }
inline std::string event_name(const void* e) { return handle_name(state().events, state().next_event, "e", e); }
inline void forget_handle(std::map<const void*, int>& m, const void* h) {
  if (!tracing()) return;
  std::lock_guard<std::mutex> lk(state().mu);
  m.erase(h);
}
// One trace line, written when it goes out of scope.
struct Line {
  std::string s;
  explicit Line(const char* what) : s(what) {}
  Line& i(const char* k, long long v) { s += ' '; s += k; s += '='; s += std::to_string(v); return *this; }
  Line& f(const char* k, double v) { char b[64]; std::snprintf(b, sizeof(b), " %s=%a", k, v); s += b; return *this; }   // bit for bit
  Line& t(const char* k, const char* text) { s += ' '; s += k; s += "=\""; s += text; s += '"'; return *this; }
  Line& p(const char* k, const void* ptr) { s += ' '; s += k; s += '='; s += ptr_name(ptr); return *this; }
  Line& st(const void* stream) { s += ' '; s += stream_name(stream); return *this; }
  Line& ev(const void* e) { s += ' '; s += event_name(e); return *this; }
  ~Line() { std::lock_guard<std::mutex> lk(state().mu); std::fprintf(state().f, "%s\n", s.c_str()); }
};
}  // namespace fake_hip

struct hipDeviceProp_t { int multiProcessorCount; char name[64]; char gcnArchName[64]; size_t totalGlobalMem; };
inline hipError_t hipGetDeviceCount(int* n) { *n = 1; return hipSuccess; }
inline hipError_t hipSetDevice(int d) { return d == 0 ? hipSuccess : hipErrorInvalidValue; }
inline hipError_t hipGetDevice(int* d) { *d = 0; return hipSuccess; }
inline hipError_t hipGetDeviceProperties(hipDeviceProp_t* p, int) {
  std::memset(p, 0, sizeof(*p));
  p->multiProcessorCount = 256;
  std::strcpy(p->name, "fake gfx950");
  std::strcpy(p->gcnArchName, "gfx950");
  return hipSuccess;
}

template <class T> inline hipError_t hipMalloc(T** p, size_t n) {
  *p = fake_hip::creation_fails() ? nullptr : static_cast<T*>(std::malloc(n ? n : 1));
  fake_hip::on_alloc(*p, n);
  return *p ? hipSuccess : hipErrorInvalidValue;
}
inline hipError_t hipFree(void* p) { fake_hip::on_free(p); std::free(p); return hipSuccess; }
inline hipError_t hipHostMalloc(void** p, size_t n, unsigned = 0) {
  *p = fake_hip::creation_fails() ? nullptr : std::malloc(n ? n : 1);
  fake_hip::on_alloc(*p, n);
  return *p ? hipSuccess : hipErrorInvalidValue;
}
inline hipError_t hipHostFree(void* p) { fake_hip::on_free(p); std::free(p); return hipSuccess; }
inline const char* fake_kind(hipMemcpyKind k) { return k == hipMemcpyHostToDevice ? "h2d" : k == hipMemcpyDeviceToHost ? "d2h" : k == hipMemcpyDeviceToDevice ? "d2d" : "h2h"; }
inline hipError_t hipMemcpy(void* d, const void* s, size_t n, hipMemcpyKind k) {
  if (fake_hip::tracing()) fake_hip::Line("memcpy").i(fake_kind(k), (long long)n).p("dst", d).p("src", s);
  std::memmove(d, s, n);
  return hipSuccess;
}
inline hipError_t hipMemcpyAsync(void* d, const void* s, size_t n, hipMemcpyKind k, hipStream_t st = nullptr) {
  if (fake_hip::tracing()) fake_hip::Line("memcpy_async").st(st).i(fake_kind(k), (long long)n).p("dst", d).p("src", s);
  std::memmove(d, s, n);
  return hipSuccess;
}
// row by row: AddressSanitizer sees both pitches
inline hipError_t hipMemcpy2DAsync(void* d, size_t dpitch, const void* s, size_t spitch, size_t width, size_t height, hipMemcpyKind k,
                                   hipStream_t st = nullptr) {
  if (fake_hip::tracing())
    fake_hip::Line("memcpy2d_async").st(st).i(fake_kind(k), (long long)width).i("height", (long long)height).i("dpitch", (long long)dpitch)
        .i("spitch", (long long)spitch).p("dst", d).p("src", s);
  for (size_t r = 0; r < height; ++r) std::memmove(static_cast<char*>(d) + r * dpitch, static_cast<const char*>(s) + r * spitch, width);
  return hipSuccess;
}
inline hipError_t hipMemset(void* d, int v, size_t n) {
  if (fake_hip::tracing()) fake_hip::Line("memset").i("bytes", (long long)n).i("value", v).p("dst", d);
  std::memset(d, v, n);
  return hipSuccess;
}
inline hipError_t hipMemsetAsync(void* d, int v, size_t n, hipStream_t st = nullptr) {
  if (fake_hip::tracing()) fake_hip::Line("memset_async").st(st).i("bytes", (long long)n).i("value", v).p("dst", d);
  std::memset(d, v, n);
  return hipSuccess;
}

inline hipError_t hipStreamCreateWithFlags(hipStream_t* s, unsigned) {
  *s = fake_hip::creation_fails() ? nullptr : new fake_stream{0};
  return *s ? hipSuccess : hipErrorInvalidValue;
}
inline hipError_t hipStreamDestroy(hipStream_t s) { fake_hip::forget_handle(fake_hip::state().streams, s); delete s; return hipSuccess; }
inline hipError_t hipStreamSynchronize(hipStream_t s) {
  if (fake_hip::tracing()) fake_hip::Line("stream_sync").st(s);
  return hipSuccess;
}
inline hipError_t hipStreamWaitEvent(hipStream_t s, hipEvent_t e, unsigned) {
  if (fake_hip::tracing()) fake_hip::Line("stream_wait").st(s).ev(e);
  return hipSuccess;
}
inline hipError_t hipDeviceGetStreamPriorityRange(int* lo, int* hi) { *lo = 1; *hi = -1; return hipSuccess; }
inline hipError_t hipStreamCreateWithPriority(hipStream_t* s, unsigned f, int) { return hipStreamCreateWithFlags(s, f); }
inline hipError_t hipEventCreate(hipEvent_t* e) {
  *e = fake_hip::creation_fails() ? nullptr : new fake_event{{}, false};
  return *e ? hipSuccess : hipErrorInvalidValue;
}
inline hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) { return hipEventCreate(e); }
inline hipError_t hipEventDestroy(hipEvent_t e) { fake_hip::forget_handle(fake_hip::state().events, e); delete e; return hipSuccess; }
inline hipError_t hipEventRecord(hipEvent_t e, hipStream_t s = nullptr) {
  if (fake_hip::tracing()) fake_hip::Line("event_record").st(s).ev(e);
  e->t = std::chrono::steady_clock::now(); e->recorded = true;
  return hipSuccess;
}
inline hipError_t hipEventSynchronize(hipEvent_t e) {
  if (fake_hip::tracing()) fake_hip::Line("event_sync").ev(e);
  return hipSuccess;
}
inline hipError_t hipEventElapsedTime(float* ms, hipEvent_t a, hipEvent_t b) {
  if (!a->recorded || !b->recorded) return hipErrorInvalidValue;
  *ms = std::chrono::duration<float, std::milli>(b->t - a->t).count();
  return hipSuccess;
}
