// Host-side handling of secrets, shared by the units that take key material (spp_witness_api.cpp: key generation and sharing;
// spp_partial_api.cpp: an auditor's share and pair seeds; spp_vss_api.cpp: a dealer's part of the key and its sharing): wiping, the operating system's randomness, and device buffers that are
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
// host scratch of secrets, wiped when it goes
struct WipedBytes {
  std::vector<uint8_t> v;
  ~WipedBytes() { wipe(v.data(), v.size()); }
};
// count field elements below r, 32 B big-endian each: 254 random bits, kept when below r (3 of 4 are)
int draw_field_elements(OsRandom& rnd, uint8_t* out, size_t count) {
  for (size_t i = 0; i < count;) {
    uint8_t* c = out + 32 * i;
    if (!rnd.next(c, 32)) return fail(SPP_ERR_IO, "cannot read /dev/urandom");
    c[0] &= 0x3f;
    if (be_is_canonical<FrParams>(c)) i++;
  }
  return SPP_OK;
}
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
