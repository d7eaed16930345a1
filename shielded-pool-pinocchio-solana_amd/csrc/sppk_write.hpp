// The two files a setup writes, from the points it computed: the SPPK proving-key container and the gnark raw verifying key.  One
// writer for spp_setup (all seven secrets from a seed, spp_setup.cpp) and spp_setup_from_ptau (no secret, spp_ptau_api.cpp), so
// that both lay a key out the same way: the sections list the same wires by the same predicates.
//   SPPK: header 7 words | alpha1 beta1 delta1 | beta2 delta2 | A: count, wires, points | B1: the same | B2: count, wires, G2 points |
//         K: count, wires, points (private wires) | Z: count, points | CB: count, wires, points (committed wires) | CS: the same
//   vk:   alpha1 beta1 | beta2 gamma2 | delta1 delta2 | count (big-endian) | K of the public wires and the challenge wire | 1 0 1 |
//         the commitment key's two G2 points
#pragma once
#include "spp_internal.hpp"

namespace {
struct KeyPoints {
  const G1Affine *A, *B1, *K, *S;          // per wire, W each: [A_j]1, [B_j]1, K_j over gamma or delta by class, sigma K_j (committed wires)
  const G2Affine* B2;                      // per wire: [B_j]2
  const G1Affine* Z;                       // n - 1 points
  G1Affine alpha1, beta1, delta1;
  G2Affine beta2, gamma2, delta2, ped_g, ped_gs;   // ped_g = rho G2, ped_gs = -rho sigma G2
};
inline void wr32(std::vector<uint8_t>& o, uint32_t v) { for (int i = 0; i < 4; i++) o.push_back((uint8_t)(v >> (8 * i))); }
inline void wr32be(std::vector<uint8_t>& o, uint32_t v) { for (int i = 3; i >= 0; i--) o.push_back((uint8_t)(v >> (8 * i))); }
inline void wr_g1(std::vector<uint8_t>& o, const G1Affine& p) { uint8_t b[64]; g1_to_raw(p, b); o.insert(o.end(), b, b + 64); }
inline void wr_g2(std::vector<uint8_t>& o, const G2Affine& p) { uint8_t b[128]; g2_to_raw(p, b); o.insert(o.end(), b, b + 128); }
inline bool write_file(const char* path, const std::vector<uint8_t>& o) {
  FILE* f = fopen(path, "wb");
  if (!f) return false;
  bool ok = fwrite(o.data(), 1, o.size(), f) == o.size();
  fclose(f);
  return ok;
}
// class of a wire in the K sums: 1 public or the challenge wire (over gamma, in the vk), 2 committed (over gamma, CB / CS), 0 private
inline std::vector<uint8_t> wire_classes(const Circuit& circ) {
  std::vector<uint8_t> cls(circ.n_wires, 0);
  for (uint32_t j = 0; j < circ.n_public; j++) cls[j] = 1;
  cls[circ.challenge_wire] = 1;
  for (uint32_t w : circ.committed) cls[w] = 2;
  return cls;
}
inline void key_files(const Circuit& circ, const std::vector<uint8_t>& cls, const KeyPoints& p, std::vector<uint8_t>& o, std::vector<uint8_t>& v) {
  const uint32_t W = circ.n_wires, n = 1u << circ.domain_log;
  wr32(o, 0x4b505053u); wr32(o, 1);
  wr32(o, circ.id); wr32(o, W); wr32(o, circ.domain_log); wr32(o, circ.n_public); wr32(o, circ.challenge_wire);
  wr_g1(o, p.alpha1); wr_g1(o, p.beta1); wr_g1(o, p.delta1); wr_g2(o, p.beta2); wr_g2(o, p.delta2);
  auto sec1 = [&](const G1Affine* pts, auto pred) {
    uint32_t cnt = 0;
    for (uint32_t j = 0; j < W; j++) cnt += pred(j) ? 1 : 0;
    wr32(o, cnt);
    for (uint32_t j = 0; j < W; j++) if (pred(j)) wr32(o, j);
    for (uint32_t j = 0; j < W; j++) if (pred(j)) wr_g1(o, pts[j]);
  };
  sec1(p.A, [&](uint32_t j) { return !p.A[j].is_inf(); });
  sec1(p.B1, [&](uint32_t j) { return !p.B1[j].is_inf(); });
  {
    uint32_t cnt = 0;
    for (uint32_t j = 0; j < W; j++) cnt += !p.B2[j].is_inf();
    wr32(o, cnt);
    for (uint32_t j = 0; j < W; j++) if (!p.B2[j].is_inf()) wr32(o, j);
    for (uint32_t j = 0; j < W; j++) if (!p.B2[j].is_inf()) wr_g2(o, p.B2[j]);
  }
  sec1(p.K, [&](uint32_t j) { return cls[j] == 0 && !p.K[j].is_inf(); });
  wr32(o, n - 1);
  for (uint32_t i = 0; i + 1 < n; i++) wr_g1(o, p.Z[i]);
  wr32(o, (uint32_t)circ.committed.size());
  for (uint32_t w : circ.committed) wr32(o, w);
  for (uint32_t w : circ.committed) wr_g1(o, p.K[w]);
  wr32(o, (uint32_t)circ.committed.size());
  for (uint32_t w : circ.committed) wr32(o, w);
  for (uint32_t w : circ.committed) wr_g1(o, p.S[w]);

  wr_g1(v, p.alpha1); wr_g1(v, p.beta1); wr_g2(v, p.beta2); wr_g2(v, p.gamma2); wr_g1(v, p.delta1); wr_g2(v, p.delta2);
  wr32be(v, circ.n_public + 1);
  for (uint32_t j = 0; j < circ.n_public; j++) wr_g1(v, p.K[j]);
  wr_g1(v, p.K[circ.challenge_wire]);
  wr32be(v, 1); wr32be(v, 0); wr32be(v, 1);
  wr_g2(v, p.ped_g); wr_g2(v, p.ped_gs);
}
}  // namespace
