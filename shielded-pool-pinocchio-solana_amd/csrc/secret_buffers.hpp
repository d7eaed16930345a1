// Host-side handling of secrets, shared by the units that take key material (spp_witness_api.cpp: key generation and sharing;
// spp_partial_api.cpp: an auditor's share and pair seeds): wiping, the operating system's randomness, and device buffers that are
// zeroed before they are freed.
#pragma once
#include "spp_internal.hpp"

namespace {
void wipe(void* p, size_t bytes) {
  volatile uint8_t* v = (volatile uint8_t*)p;
  for (size_t i = 0; i < bytes; i++) v[i] = 0;
}
// OS randomness in blocks; wiped when it goes
struct OsRandom {
  FILE* f = nullptr;
  uint8_t buf[4096];
  size_t pos = sizeof buf;
  ~OsRandom() {
    if (f) fclose(f);
    wipe(buf, sizeof buf);
  }
  bool next(uint8_t* out, size_t n) {
    for (size_t i = 0; i < n; i++) {
      if (pos == sizeof buf) {
        if (!f) {
          f = fopen("/dev/urandom", "rb");
          if (f) setvbuf(f, nullptr, _IONBF, 0);   // no second copy of the bytes in a stdio buffer
        }
        if (!f || fread(buf, 1, sizeof buf, f) != sizeof buf) return false;
        pos = 0;
      }
      out[i] = buf[pos++];
    }
    return true;
  }
};
// device buffer of secrets: zeroed on its stream before DevBuf's destructor frees it, on every return path
struct WipedDevBuf : DevBuf {
  size_t bytes = 0;
  hipStream_t st = nullptr;
  ~WipedDevBuf() {
    if (p && bytes) {
      (void)hipMemsetAsync(p, 0, bytes, st);
      (void)hipStreamSynchronize(st);
    }
  }
};
#define UP_SECRET(buf, src, nbytes) \
  do {                              \
    buf.bytes = (nbytes);           \
    buf.st = st;                    \
    UP(buf, src, nbytes);           \
  } while (0)
}  // namespace
