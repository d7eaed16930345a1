// libspp C ABI (include/spp.h), core: the error channel and contexts.  Circuit loading is spp_load.cpp, the batched proving
// pipeline spp_prove.cpp, the trusted setup spp_setup.cpp.  Everything heavy runs on the GPU; the host parses containers,
// derives one-time constants and enqueues kernels.  There is deliberately no CPU implementation of the hot path here.
#include "spp_internal.hpp"
#include <chrono>

thread_local char g_spp_err[512] = "";
extern "C" const char* spp_last_error(void) { return g_spp_err; }
extern "C" const char* spp_version(void) { return "libspp 0.2 (gfx950)"; }

// -----------------------------------------------------------------------------------------------------
// context
// -----------------------------------------------------------------------------------------------------
extern "C" int spp_init(int device, spp_ctx** out) {
  if (!out) return fail(SPP_ERR_BAD_INPUT, "out is NULL");
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
    return fail(SPP_ERR_NO_DEVICE, "no HIP device visible: libspp has no CPU fallback");
  if (device < 0 || device >= count) return fail(SPP_ERR_NO_DEVICE, "device %d out of range (%d visible)", device, count);
  HIP_TRY(hipSetDevice(device));
  spp_ctx* ctx = new spp_ctx();
  ctx->device = device;
  ctx->stream = nullptr;
  for (int k = 0; k < SPP_NWS; k++) ctx->pstream[k] = nullptr;
  struct Guard {   // a failure below must not leak the context and the streams created so far
    spp_ctx* ctx;
    ~Guard() { if (ctx) spp_free_ctx(ctx); }
  } guard{ctx};
  HIP_TRY(hipStreamCreate(&ctx->stream));
  HIP_TRY(hipStreamCreate(&ctx->pstream[0]));
  for (int k = 1; k < SPP_NWS; k++)
    if (int e = pick_concurrent_stream(ctx->pstream[0], &ctx->pstream[k])) return e;
  guard.ctx = nullptr;
  *out = ctx;
  return SPP_OK;
}
// A new stream that really runs beside `ref`.  HIP multiplexes the streams of one priority onto a few hardware queues in
// creation order; two streams that share a queue execute in submission order, and which ones do depends on how many streams
// the process (torch included) created before -- seen as run-to-run differences of 4 % on pipelined batches and 0.5 ms on a
// single proof whose G2 sum ran in front of the matrix evaluation instead of beside it.  Probe: a one-lane kernel that waits
// 2 ms on `ref`, a trivial kernel on the candidate; the candidate is kept if its kernel finishes while the other still waits.
int pick_concurrent_stream(hipStream_t ref, hipStream_t* out) {
  static const bool probe = getenv("SPP_NO_STREAM_PROBE") == nullptr;
  hipStream_t rejected[6];
  int nrej = 0;
  *out = nullptr;
  for (int attempt = 0; attempt < 6 && probe; attempt++) {
    hipStream_t cand;
    HIP_TRY(hipStreamCreate(&cand));
    HIP_TRY(hipStreamSynchronize(ref));
    launch_spin(ref, 200000, nullptr);            // 2 ms of the 100 MHz wall clock
    const auto t0 = std::chrono::steady_clock::now();
    launch_touch(cand, nullptr);
    HIP_TRY(hipStreamSynchronize(cand));
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    HIP_TRY(hipStreamSynchronize(ref));
    if (ms < 1.0) {
      *out = cand;
      break;
    }
    rejected[nrej++] = cand;                      // keep it alive until the search ends: destroying it would free its queue slot
  }
  for (int i = 0; i < nrej; i++) hipStreamDestroy(rejected[i]);
  if (!*out) HIP_TRY(hipStreamCreate(out));
  return 0;
}

extern "C" void spp_free_ctx(spp_ctx* ctx) {
  if (!ctx) return;
  hipSetDevice(ctx->device);
  if (ctx->stream) hipStreamDestroy(ctx->stream);
  for (int k = 0; k < SPP_NWS; k++)
    if (ctx->pstream[k]) hipStreamDestroy(ctx->pstream[k]);
  for (void* p : ctx->owned) hipFree(p);
  if (ctx->audit_scratch) hipFree(ctx->audit_scratch);
  delete ctx;
}

