// libspp C ABI, the setup ceremony's first phase: the powers-of-tau transcript (new, contribute, verify one link), the derivation of a
// circuit's keys from it, and the unit entry points of their kernels (include/spp.h has the protocol; ptau.hpp the container, the
// host planning and the kernels' method).
#include "spp_internal.hpp"
#include "ceremony_host.hpp"
#include "ptau.hpp"
#include "sppk_write.hpp"

#include <chrono>
#include <thread>

namespace {
// what tells the two groups apart on the way from raw bytes to the kernels and back
template <class F>
struct RawPoint;
template <>
struct RawPoint<Fq> {
  static constexpr size_t size = 64;
  static void to_raw(const G1Affine& p, uint8_t* b) { g1_to_raw(p, b); }
  static void launch_mul_each(hipStream_t st, const G1Affine* p, uint32_t n, const uint32_t* sc, G1Affine* o) { launch_g1_mul_each(st, p, n, sc, o); }
  static void launch_decode(hipStream_t st, const uint8_t* raw, uint32_t n, G1Affine* pts, uint32_t* flags) {
    launch_g1_decode_check(st, raw, n, pts, flags);
  }
};
template <>
struct RawPoint<Fq2> {
  static constexpr size_t size = 128;
  static void to_raw(const G2Affine& p, uint8_t* b) { g2_to_raw(p, b); }
  static void launch_mul_each(hipStream_t st, const G2Affine* p, uint32_t n, const uint32_t* sc, G2Affine* o) { launch_g2_mul_each(st, p, n, sc, o); }
  static void launch_decode(hipStream_t st, const uint8_t* raw, uint32_t n, G2Affine* pts, uint32_t* flags) {
    launch_g2_decode_check(st, raw, n, twist_b(), pts, flags);
  }
};
// raw[n] -> d_pts (Montgomery form) and flags (host): range and curve checks on the device.  ctx->mu held, device set.
template <class F>
int decode_raw(hipStream_t st, const uint8_t* raw, size_t n, DevBuf& d_pts, std::vector<uint32_t>& flags) {
  DevBuf d_raw, d_flags;
  UP(d_raw, raw, n * RawPoint<F>::size);
  HIP_TRY(d_pts.alloc(n * sizeof(Affine<F>)));
  HIP_TRY(d_flags.alloc(n * sizeof(uint32_t)));
  RawPoint<F>::launch_decode(st, d_raw.as<uint8_t>(), (uint32_t)n, d_pts.as<Affine<F>>(), d_flags.as<uint32_t>());
  HIP_TRY(hipGetLastError());
  flags.resize(n);
  if (n) HIP_TRY(hipMemcpyAsync(flags.data(), d_flags.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return SPP_OK;
}
// out[i] = d_sc[i] * d_pts[i] as raw bytes; d_sc: 8 canonical words per point, on the device
template <class F>
int mul_each_to_raw(hipStream_t st, DevBuf& d_pts, size_t n, const uint32_t* d_sc, uint8_t* out) {
  if (n == 0) return SPP_OK;
  DevBuf d_out;
  HIP_TRY(d_out.alloc(n * sizeof(Affine<F>)));
  RawPoint<F>::launch_mul_each(st, d_pts.as<Affine<F>>(), (uint32_t)n, d_sc, d_out.as<Affine<F>>());
  HIP_TRY(hipGetLastError());
  std::vector<Affine<F>> res(n);
  HIP_TRY(hipMemcpyAsync(res.data(), d_out.p, n * sizeof(Affine<F>), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (size_t i = 0; i < n; i++) RawPoint<F>::to_raw(res[i], out + RawPoint<F>::size * i);
  return SPP_OK;
}
// every one of the n raw G2 points lies in the order-r subgroup (the points passed the device's curve check); one [r]Q per
// point, cut over a few host threads: at n = 2^14 one thread needs seconds
bool g2_all_in_subgroup(const uint8_t* raw, size_t n) {
  const size_t nt = std::max<size_t>(1, std::min<size_t>({(size_t)8, (size_t)std::thread::hardware_concurrency(), n / 64 + 1}));
  std::vector<int> good(nt, 1);
  auto work = [&](size_t t) {
    for (size_t i = t; i < n; i += nt)
      if (!g2_in_subgroup(g2_from_raw(raw + 128 * i))) { good[t] = 0; return; }
  };
  std::vector<std::thread> th;
  for (size_t t = 1; t < nt; t++) th.emplace_back(work, t);
  work(0);
  for (auto& x : th) x.join();
  return std::all_of(good.begin(), good.end(), [](int g) { return g != 0; });
}
// c of one of a transcript receipt's three proofs
Fr ptau_challenge(const uint8_t file_hash[32], const uint8_t* base, const uint8_t* base_after, const uint8_t* T) {
  uint8_t m[32 + 3 * 64];
  memcpy(m, file_hash, 32);
  memcpy(m + 32, base, 64);
  memcpy(m + 96, base_after, 64);
  memcpy(m + 160, T, 64);
  Fr c;
  hash_to_fr(m, sizeof m, "spp-ptau-contribute-c1", &c, 1);
  return c;
}
// the three (secret, base) pairs of a receipt: (t, T1_1), (a, A1_0), (b, B1_0) as byte offsets into a transcript
void receipt_bases(const PtauLayout& L, size_t at[3]) {
  at[0] = L.t1 + 64;
  at[1] = L.a1;
  at[2] = L.b1;
}
// rho_i of the ratio tests: the first 128 bits of SHA256(hash before | hash after | tag | i as 8 bytes big-endian)
enum : uint8_t { PT_TAG_T1 = 1, PT_TAG_T2 = 2, PT_TAG_A1 = 3, PT_TAG_B1 = 4 };
std::vector<Fr> ratio_scalars(const uint8_t hb[32], const uint8_t ha[32], uint8_t tag, size_t count) {
  std::vector<Fr> rho(count);
  uint8_t m[73], dg[32];
  memcpy(m, hb, 32);
  memcpy(m + 32, ha, 32);
  m[64] = tag;
  for (size_t i = 0; i < count; i++) {
    for (int b = 0; b < 8; b++) m[65 + b] = (uint8_t)((uint64_t)i >> (8 * (7 - b)));
    sha256_bytes(m, sizeof m, dg);
    uint32_t w[8] = {sc_load_be32(dg + 12), sc_load_be32(dg + 8), sc_load_be32(dg + 4), sc_load_be32(dg), 0, 0, 0, 0};
    rho[i] = Fr::from_canonical(w);
  }
  return rho;
}
// hi = sum rho_i pts[i + 1], lo = sum rho_i pts[i], i < count, over device-resident points (count + 1 of them)
int ratio_sums(hipStream_t st, const G1Affine* d_pts, const std::vector<Fr>& rho, DevBuf& d_ws, G1Affine* hi, G1Affine* lo) {
  DevBuf d_rho;
  UP(d_rho, rho.data(), rho.size() * sizeof(Fr));
  G1Affine* out[2] = {lo, hi};
  for (int side = 0; side < 2; side++) {
    G1XYZZ* win = nullptr;
    launch_pippenger_g1(st, d_pts + side, d_rho.as<Fr>(), (uint32_t)rho.size(), d_ws.p, &win, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    if (int e = pippenger_sum(win, out[side])) return e;
  }
  return SPP_OK;
}
int ratio_sums_g2(hipStream_t st, const G2Affine* d_pts, const std::vector<Fr>& rho, G2Affine* hi, G2Affine* lo) {
  DevBuf d_rho, d_ws;
  UP(d_rho, rho.data(), rho.size() * sizeof(Fr));
  HIP_TRY(d_ws.alloc(pippenger_workspace_bytes_g2((uint32_t)rho.size())));
  G2Affine* out[2] = {lo, hi};
  for (int side = 0; side < 2; side++) {
    G2XYZZ* win = nullptr;
    launch_pippenger_g2(st, d_pts + side, d_rho.as<Fr>(), (uint32_t)rho.size(), d_ws.p, &win, nullptr, nullptr);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    if (int e = pippenger_sum(win, out[side])) return e;
  }
  return SPP_OK;
}

// the unit entry points: scalars_be n * 32 B, each 0 < k < r
template <class F>
int mul_each_unit(spp_ctx* ctx, const uint8_t* points, size_t n, const uint8_t* scalars_be, uint8_t* out) {
  if (!ctx || (n && (!points || !scalars_be || !out))) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (n >= (1u << 28)) return fail(SPP_ERR_BAD_INPUT, "too many points");
  std::vector<uint32_t> sc(8 * n);
  Wipe wsc{sc.data(), sc.size() * sizeof(uint32_t)};
  for (size_t i = 0; i < n; i++) {
    for (int k = 0; k < 8; k++) sc[8 * i + 7 - k] = sc_load_be32(scalars_be + 32 * i + 4 * k);
    if (!pt_scalar_ok(&sc[8 * i])) return fail(SPP_ERR_BAD_INPUT, "scalar %zu is zero or not below r", i);
  }
  if (n == 0) return SPP_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf d_pts, d_sc;
  std::vector<uint32_t> flags;
  if (int e = decode_raw<F>(st, points, n, d_pts, flags)) return e;
  for (size_t i = 0; i < n; i++)
    if (flags[i] == SC_POINT_BAD) return fail(SPP_ERR_BAD_INPUT, "point %zu is not on the curve", i);
  HIP_TRY(d_sc.alloc(sc.size() * sizeof(uint32_t)));
  DevWipe dw{d_sc, sc.size() * sizeof(uint32_t), st};
  HIP_TRY(hipMemcpyAsync(d_sc.p, sc.data(), sc.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
  return mul_each_to_raw<F>(st, d_pts, n, d_sc.as<uint32_t>(), out);
}
}  // namespace

extern "C" int spp_g1_mul_each(spp_ctx* ctx, const uint8_t* points, size_t n, const uint8_t* scalars_be, uint8_t* out) {
  return mul_each_unit<Fq>(ctx, points, n, scalars_be, out);
}
extern "C" int spp_g2_mul_each(spp_ctx* ctx, const uint8_t* points, size_t n, const uint8_t* scalars_be, uint8_t* out) {
  return mul_each_unit<Fq2>(ctx, points, n, scalars_be, out);
}

extern "C" int spp_ptau_new(uint32_t domain_log, const char* path) {
  if (!path) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  PtauLayout L;
  if (!ptau_layout_of(domain_log, &L)) return fail(SPP_ERR_BAD_INPUT, "domain_log %u is not in [1, %u]", domain_log, PT_MAX_LOG);
  std::vector<uint8_t> o(L.size);
  pt_store_le32(o.data(), PT_MAGIC);
  pt_store_le32(o.data() + 4, 1);
  pt_store_le32(o.data() + 8, domain_log);
  uint8_t g1[64], g2[128];
  g1_to_raw(g1_generator(), g1);
  g2_to_raw(g2_generator(), g2);
  for (size_t i = 0; i < L.n_t1; i++) memcpy(o.data() + L.t1 + 64 * i, g1, 64);
  for (size_t i = 0; i < L.n; i++) {
    memcpy(o.data() + L.t2 + 128 * i, g2, 128);
    memcpy(o.data() + L.a1 + 64 * i, g1, 64);
    memcpy(o.data() + L.b1 + 64 * i, g1, 64);
  }
  memcpy(o.data() + L.beta2, g2, 128);
  if (!write_bytes(path, o.data(), o.size())) return fail(SPP_ERR_IO, "cannot write %s", path);
  return SPP_OK;
}

extern "C" int spp_ptau_contribute(spp_ctx* ctx, const char* in_path, const uint8_t entropy[32], const char* out_path,
                                   uint8_t receipt[SPP_PTAU_RECEIPT_LEN]) {
  if (!ctx || !in_path || !out_path || !receipt) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  std::vector<uint8_t> in;
  if (!read_file(in_path, in)) return fail(SPP_ERR_IO, "cannot read %s", in_path);
  PtauLayout L;
  if (!ptau_layout(in.data(), in.size(), &L)) return fail(SPP_ERR_FORMAT, "%s is not a transcript", in_path);
  const size_t n = L.n, n_g1 = (size_t)L.n_t1 + 2 * n;

  // the secrets t, a, b, the receipt's nonces and everything computed from them: cleared on every path
  uint8_t seed[32];
  Fr s[6], pw, prod;
  uint32_t limbs[8];
  std::vector<uint32_t> sc(8 * n_g1);   // [t^i, i < 2n - 1 | a t^i, i < n | b t^i, i < n]; T2 takes the first n rows
  Wipe w0{seed, sizeof seed}, w1{s, sizeof s}, w2{&pw, sizeof pw}, w3{&prod, sizeof prod}, w4{limbs, sizeof limbs},
      w5{sc.data(), sc.size() * sizeof(uint32_t)};
  if (!ceremony_seed(entropy, seed)) return fail(SPP_ERR_IO, "no randomness from the operating system");
  hash_to_fr(seed, 32, "spp-ptau-contribute-v1", s, 6);
  if (s[0].is_zero() || s[1].is_zero() || s[2].is_zero()) return fail(SPP_ERR_BAD_INPUT, "the entropy gives a contribution zero: use another");
  pw = Fr::one();
  for (size_t i = 0; i < L.n_t1; i++) {
    pw.to_canonical(&sc[8 * i]);
    if (i < n) {
      prod = s[1] * pw;
      prod.to_canonical(&sc[8 * (L.n_t1 + i)]);
      prod = s[2] * pw;
      prod.to_canonical(&sc[8 * (L.n_t1 + n + i)]);
    }
    pw = pw * s[0];
  }

  // every point of the input is a point before anything multiplies it: range and curve on the device, the subgroup of the G2
  // points on the host; infinity has no place in a transcript
  std::vector<uint8_t> g1_raw(n_g1 * 64);   // T1 | A1 | B1 (A1 and B1 are neighbours in the file)
  memcpy(g1_raw.data(), in.data() + L.t1, (size_t)L.n_t1 * 64);
  memcpy(g1_raw.data() + (size_t)L.n_t1 * 64, in.data() + L.a1, 2 * n * 64);
  std::vector<uint8_t> out = in;
  G2Affine beta2;
  if (!g2_raw_valid(in.data() + L.beta2, &beta2)) return fail(SPP_ERR_FORMAT, "%s: beta2 is not a point of the group", in_path);
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf d_g1, d_g2, d_sc;
    std::vector<uint32_t> f1, f2;
    if (int e = decode_raw<Fq>(st, g1_raw.data(), n_g1, d_g1, f1)) return e;
    if (int e = decode_raw<Fq2>(st, in.data() + L.t2, n, d_g2, f2)) return e;
    for (size_t i = 0; i < n_g1; i++)
      if (f1[i] != SC_POINT_OK) return fail(SPP_ERR_FORMAT, "%s: G1 point %zu (T1 | A1 | B1) is not a point of the curve", in_path, i);
    for (size_t i = 0; i < n; i++)
      if (f2[i] != SC_POINT_OK) return fail(SPP_ERR_FORMAT, "%s: T2 point %zu is not a point of the twist", in_path, i);
    if (!g2_all_in_subgroup(in.data() + L.t2, n)) return fail(SPP_ERR_FORMAT, "%s: a T2 point is outside the order-r subgroup", in_path);
    uint8_t g1[64], g2[128];
    g1_to_raw(g1_generator(), g1);
    g2_to_raw(g2_generator(), g2);
    if (memcmp(in.data() + L.t1, g1, 64) != 0 || memcmp(in.data() + L.t2, g2, 128) != 0)
      return fail(SPP_ERR_FORMAT, "%s: the powers do not start at the generators", in_path);

    // one upload of the scalars, one launch per group
    HIP_TRY(d_sc.alloc(sc.size() * sizeof(uint32_t)));
    DevWipe dw{d_sc, sc.size() * sizeof(uint32_t), st};
    HIP_TRY(hipMemcpyAsync(d_sc.p, sc.data(), sc.size() * sizeof(uint32_t), hipMemcpyHostToDevice, st));
    if (int e = mul_each_to_raw<Fq>(st, d_g1, n_g1, d_sc.as<uint32_t>(), g1_raw.data())) return e;
    if (int e = mul_each_to_raw<Fq2>(st, d_g2, n, d_sc.as<uint32_t>(), out.data() + L.t2)) return e;
  }
  memcpy(out.data() + L.t1, g1_raw.data(), (size_t)L.n_t1 * 64);
  memcpy(out.data() + L.a1, g1_raw.data() + (size_t)L.n_t1 * 64, 2 * n * 64);
  s[2].to_canonical(limbs);
  g2_to_raw(scalar_mul(beta2, limbs).to_affine(), out.data() + L.beta2);

  // the receipt: knowledge of t, a and b, each bound to the file it was applied to
  uint8_t file_hash[32];
  sha256_bytes(in.data(), in.size(), file_hash);
  size_t at[3];
  receipt_bases(L, at);
  for (int j = 0; j < 3; j++) {
    uint8_t* r = receipt + 160 * j;
    G1Affine base;
    sc_decode_point(in.data() + at[j], &base);
    s[3 + j].to_canonical(limbs);
    memcpy(r, out.data() + at[j], 64);
    g1_to_raw(scalar_mul(base, limbs).to_affine(), r + 64);
    const Fr c = ptau_challenge(file_hash, in.data() + at[j], r, r + 64);
    const Fr z = s[3 + j] + c * s[j];   // public
    z.to_bytes_be(r + 128);
  }
  if (!write_bytes(out_path, out.data(), out.size())) return fail(SPP_ERR_IO, "cannot write %s", out_path);
  return SPP_OK;
}

extern "C" int spp_ptau_verify_contribution(spp_ctx* ctx, const char* before_path, const char* after_path,
                                            const uint8_t receipt[SPP_PTAU_RECEIPT_LEN], int* ok, uint32_t* reason) {
  if (!ctx || !before_path || !after_path || !receipt || !ok || !reason) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  *ok = 0;
  *reason = SPP_PTAU_FORMAT;
  std::vector<uint8_t> fb, fa;
  if (!read_file(before_path, fb)) return fail(SPP_ERR_IO, "cannot read %s", before_path);
  if (!read_file(after_path, fa)) return fail(SPP_ERR_IO, "cannot read %s", after_path);
  auto refuse = [&](uint32_t why) { *reason = why; return SPP_OK; };

  // 1., 2. both files parse, at one size
  PtauLayout Lb, L;
  if (!ptau_layout(fb.data(), fb.size(), &Lb) || !ptau_layout(fa.data(), fa.size(), &L)) return refuse(SPP_PTAU_FORMAT);
  if (Lb.log != L.log) return refuse(SPP_PTAU_SIZE);
  const size_t n = L.n, n_g1 = (size_t)L.n_t1 + 2 * n;

  // 3. every point of the transcript after is a point, none is infinity, the powers start at the generators; T2'_1, beta2' and
  //    the two combinations of the T2' points that the ratio test pairs lie in the order-r subgroup
  std::vector<uint8_t> g1_raw(n_g1 * 64);
  memcpy(g1_raw.data(), fa.data() + L.t1, (size_t)L.n_t1 * 64);
  memcpy(g1_raw.data() + (size_t)L.n_t1 * 64, fa.data() + L.a1, 2 * n * 64);
  uint8_t hb[32], ha[32];
  sha256_bytes(fb.data(), fb.size(), hb);
  sha256_bytes(fa.data(), fa.size(), ha);
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf d_g1, d_g2;
  {
    std::vector<uint32_t> f1, f2;
    if (int e = decode_raw<Fq>(st, g1_raw.data(), n_g1, d_g1, f1)) return e;
    if (int e = decode_raw<Fq2>(st, fa.data() + L.t2, n, d_g2, f2)) return e;
    for (uint32_t f : f1)
      if (f != SC_POINT_OK) return refuse(SPP_PTAU_POINT_INVALID);
    for (uint32_t f : f2)
      if (f != SC_POINT_OK) return refuse(SPP_PTAU_POINT_INVALID);
  }
  const G1Affine g1 = g1_generator();
  const G2Affine g2 = g2_generator();
  {
    uint8_t g1b[64], g2b[128];
    g1_to_raw(g1, g1b);
    g2_to_raw(g2, g2b);
    if (memcmp(fa.data() + L.t1, g1b, 64) != 0 || memcmp(fa.data() + L.t2, g2b, 128) != 0) return refuse(SPP_PTAU_POINT_INVALID);
  }
  G2Affine tau2, beta2, s2_hi, s2_lo;
  if (!g2_raw_valid(fa.data() + L.t2 + 128, &tau2) || !g2_raw_valid(fa.data() + L.beta2, &beta2)) return refuse(SPP_PTAU_POINT_INVALID);
  if (int e = ratio_sums_g2(st, d_g2.as<G2Affine>(), ratio_scalars(hb, ha, PT_TAG_T2, n - 1), &s2_hi, &s2_lo)) return e;
  if (!g2_in_subgroup(s2_hi) || !g2_in_subgroup(s2_lo)) return refuse(SPP_PTAU_POINT_INVALID);

  // 4. the receipt: knowledge of t, a, b with T1'_1 = t T1_1, A1'_0 = a A1_0, B1'_0 = b B1_0
  size_t at[3];
  receipt_bases(L, at);
  for (int j = 0; j < 3; j++) {
    const uint8_t* r = receipt + 160 * j;
    G1Affine base, base_after, T;
    if (memcmp(r, fa.data() + at[j], 64) != 0) return refuse(SPP_PTAU_RECEIPT);
    if (sc_decode_point(fb.data() + at[j], &base) != SC_POINT_OK || sc_decode_point(r, &base_after) != SC_POINT_OK) return refuse(SPP_PTAU_RECEIPT);
    if (sc_decode_point(r + 64, &T) == SC_POINT_BAD || !be_is_canonical<FrParams>(r + 128)) return refuse(SPP_PTAU_RECEIPT);
    if (!schnorr_holds(base, base_after, T, ptau_challenge(hb, fb.data() + at[j], r, r + 64), r + 128)) return refuse(SPP_PTAU_RECEIPT);
  }

  // 5. - 8. consecutive points of each section differ by the factor tau' that T2'_1 (for G1) and T1'_1 (for G2) hold
  DevBuf d_ws;
  HIP_TRY(d_ws.alloc(pippenger_workspace_bytes((uint32_t)L.n_t1)));
  const G1Affine* T1 = d_g1.as<G1Affine>();
  G1Affine hi, lo, tau1, b1_0;
  sc_decode_point(fa.data() + L.t1 + 64, &tau1);
  sc_decode_point(fa.data() + L.b1, &b1_0);
  if (int e = ratio_sums(st, T1, ratio_scalars(hb, ha, PT_TAG_T1, (size_t)L.n_t1 - 1), d_ws, &hi, &lo)) return e;
  if (!pairing_is_one({{hi, g2}, {lo.neg(), tau2}})) return refuse(SPP_PTAU_TAU_G1);
  if (s2_lo.is_inf() || s2_hi.is_inf() || !pairing_is_one({{tau1, s2_lo}, {g1.neg(), s2_hi}})) return refuse(SPP_PTAU_TAU_G2);
  if (int e = ratio_sums(st, T1 + L.n_t1, ratio_scalars(hb, ha, PT_TAG_A1, n - 1), d_ws, &hi, &lo)) return e;
  if (!pairing_is_one({{hi, g2}, {lo.neg(), tau2}})) return refuse(SPP_PTAU_ALPHA);
  if (int e = ratio_sums(st, T1 + L.n_t1 + n, ratio_scalars(hb, ha, PT_TAG_B1, n - 1), d_ws, &hi, &lo)) return e;
  if (!pairing_is_one({{hi, g2}, {lo.neg(), tau2}}) || !pairing_is_one({{b1_0, g2}, {g1.neg(), beta2}})) return refuse(SPP_PTAU_BETA);
  *ok = 1;
  *reason = SPP_PTAU_OK;
  return SPP_OK;
}

// -----------------------------------------------------------------------------------------------------
// the group inverse NTT and the derivation of a circuit's keys from a transcript
// -----------------------------------------------------------------------------------------------------
namespace {
// d_out[b][k] = (1 / n) sum_i w^(-k i) d_in[b][i] for nbatch transforms of n = 2^logn points, w = fr_root_of_unity(logn), the root
// spp_setup takes; waits for the stream, so that the tables and the work arrays are released with the call.  ms (optional):
// the stages, then the scaling by 1 / n
template <class F>
int intt_on_device(hipStream_t st, const Affine<F>* d_in, uint32_t logn, uint32_t nbatch, Affine<F>* d_out, float ms[2] = nullptr) {
  const uint32_t n = 1u << logn;
  std::vector<uint32_t> tw((size_t)8 * (n / 2));
  const Fr winv = fr_root_of_unity(logn).inv();
  Fr p = Fr::one();
  for (uint32_t j = 0; j < n / 2; j++) {
    p.to_canonical(&tw[(size_t)8 * j]);
    p = p * winv;
  }
  uint32_t ninv[8];
  int8_t dig[SC_MAX_DIGITS];
  Fr::from_u64(n).inv().to_canonical(ninv);
  const uint32_t len = sc_naf_recode(ninv, dig);
  DevBuf d_tw, d_dig, d_work;
  UP(d_tw, tw.data(), tw.size() * sizeof(uint32_t));
  UP(d_dig, dig, sizeof dig);
  HIP_TRY(d_work.alloc((size_t)2 * nbatch * n * sizeof(XYZZ<F>)));
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  if (ms) {
    for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
    hipEventRecord(ev[0], st);
  }
  launch_ec_intt<F>(st, d_in, d_work.as<XYZZ<F>>(), logn, nbatch, d_tw.as<uint32_t>(), d_dig.as<int8_t>(), len, d_out, ev[1], ev[2]);
  const hipError_t launched = hipGetLastError(), done = hipStreamSynchronize(st);
  if (ms) {
    if (launched == hipSuccess && done == hipSuccess) {
      hipEventElapsedTime(&ms[0], ev[0], ev[1]);
      hipEventElapsedTime(&ms[1], ev[1], ev[2]);
    }
    for (auto& e : ev) hipEventDestroy(e);
  }
  HIP_TRY(launched);
  HIP_TRY(done);
  return SPP_OK;
}
// ms (optional): the stages and the scaling between events; host_ms (optional): one host thread over the first host_butterflies
// butterflies of stage 0, the text the lanes run (pt_bfly_sum, pt_bfly_diff with the twiddle of the butterfly's index)
template <class F>
int intt_unit(spp_ctx* ctx, const uint8_t* points, uint32_t logn, uint8_t* out, float* ms = nullptr, size_t host_butterflies = 0,
              float* host_ms = nullptr) {
  if (!ctx || !points || !out) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (logn == 0 || logn > PT_MAX_LOG) return fail(SPP_ERR_BAD_INPUT, "logn %u is not in [1, %u]", logn, PT_MAX_LOG);
  const size_t n = (size_t)1 << logn;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf d_in, d_out;
  std::vector<uint32_t> flags;
  if (int e = decode_raw<F>(st, points, n, d_in, flags)) return e;
  for (size_t i = 0; i < n; i++)
    if (flags[i] == SC_POINT_BAD) return fail(SPP_ERR_BAD_INPUT, "point %zu is not on the curve", i);
  HIP_TRY(d_out.alloc(n * sizeof(Affine<F>)));
  if (int e = intt_on_device<F>(st, d_in.as<Affine<F>>(), logn, 1, d_out.as<Affine<F>>(), ms)) return e;
  if (host_ms) {
    const size_t m = std::min(host_butterflies, n / 2);
    std::vector<Affine<F>> in(n);
    HIP_TRY(hipMemcpy(in.data(), d_in.p, n * sizeof(Affine<F>), hipMemcpyDeviceToHost));
    const Fr winv = fr_root_of_unity(logn).inv();
    std::vector<uint32_t> tw(8 * std::max<size_t>(m, 1));
    Fr p = Fr::one();
    for (size_t j = 0; j < m; j++) {
      p.to_canonical(&tw[8 * j]);
      p = p * winv;
    }
    std::vector<XYZZ<F>> sink(2 * std::max<size_t>(m, 1));
    const auto t0 = std::chrono::steady_clock::now();
    for (size_t j = 0; j < m; j++) {
      const XYZZ<F> a = XYZZ<F>::from_affine(in[j]), b = XYZZ<F>::from_affine(in[j + n / 2]);
      sink[2 * j] = pt_bfly_sum(a, b);
      sink[2 * j + 1] = pt_bfly_diff(a, b, &tw[8 * j], j == 0);
    }
    *host_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
  }
  std::vector<Affine<F>> res(n);
  HIP_TRY(hipMemcpy(res.data(), d_out.p, n * sizeof(Affine<F>), hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; i++) RawPoint<F>::to_raw(res[i], out + RawPoint<F>::size * i);
  return SPP_OK;
}
// out (host, ncols points) = the gather of `entries` over the device-resident bases
template <class F>
int gather_on_device(hipStream_t st, const Affine<F>* d_bases, uint32_t nbases, uint32_t ncols, const std::vector<ColEntry>& entries,
                     const uint32_t* d_mags, const uint32_t* d_meta, uint32_t ncoef, std::vector<Affine<F>>& out) {
  ColPlan plan;
  if (!col_plan(ncols, nbases, ncoef, entries, &plan)) return fail(SPP_ERR_FORMAT, "the circuit names a wire, a constraint or a coefficient out of range");
  const uint32_t nchunks = (uint32_t)plan.chunk_ptr.size() - 1;
  DevBuf d_terms, d_chunk, d_col, d_partial, d_out;
  UP(d_terms, plan.terms.data(), plan.terms.size() * sizeof(uint32_t));
  UP(d_chunk, plan.chunk_ptr.data(), plan.chunk_ptr.size() * sizeof(uint32_t));
  UP(d_col, plan.col_ptr.data(), plan.col_ptr.size() * sizeof(uint32_t));
  HIP_TRY(d_partial.alloc((size_t)nchunks * sizeof(XYZZ<F>)));
  HIP_TRY(d_out.alloc((size_t)ncols * sizeof(Affine<F>)));
  launch_col_gather<F>(st, d_bases, d_terms.as<uint32_t>(), d_chunk.as<uint32_t>(), nchunks, d_col.as<uint32_t>(), ncols, d_mags, d_meta,
                       d_partial.as<XYZZ<F>>(), d_out.as<Affine<F>>());
  HIP_TRY(hipGetLastError());
  out.resize(ncols);
  if (ncols) HIP_TRY(hipMemcpyAsync(out.data(), d_out.p, (size_t)ncols * sizeof(Affine<F>), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return SPP_OK;
}
}  // namespace

extern "C" int spp_ec_intt_g1(spp_ctx* ctx, const uint8_t* points, uint32_t logn, uint8_t* out) { return intt_unit<Fq>(ctx, points, logn, out); }
extern "C" int spp_ec_intt_g2(spp_ctx* ctx, const uint8_t* points, uint32_t logn, uint8_t* out) { return intt_unit<Fq2>(ctx, points, logn, out); }

extern "C" int spp_ec_intt_timed(spp_ctx* ctx, int group, const uint8_t* points, uint32_t logn, uint8_t* out, float ms[2], size_t host_butterflies,
                                 float* host_ms) {
  if (group != 1 && group != 2) return fail(SPP_ERR_BAD_INPUT, "group is 1 (G1) or 2 (G2)");
  return group == 1 ? intt_unit<Fq>(ctx, points, logn, out, ms, host_butterflies, host_ms) : intt_unit<Fq2>(ctx, points, logn, out, ms, host_butterflies, host_ms);
}

extern "C" int spp_setup_from_ptau(spp_ctx* ctx, const char* circuit_path, const char* ptau_path, const char* pk_path, const char* vk_path) {
  if (!ctx || !circuit_path || !ptau_path || !pk_path || !vk_path) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  Circuit circ;
  if (!circ.load(circuit_path)) return fail(SPP_ERR_IO, "cannot read circuit %s", circuit_path);
  std::vector<uint8_t> pt;
  if (!read_file(ptau_path, pt)) return fail(SPP_ERR_IO, "cannot read %s", ptau_path);
  PtauLayout L;
  if (!ptau_layout(pt.data(), pt.size(), &L)) return fail(SPP_ERR_FORMAT, "%s is not a transcript", ptau_path);
  const uint32_t logn = circ.domain_log, W = circ.n_wires;
  if (logn == 0 || logn > PT_MAX_LOG) return fail(SPP_ERR_FORMAT, "%s: domain_log %u is not in [1, %u]", circuit_path, logn, PT_MAX_LOG);
  if (L.log < logn) return fail(SPP_ERR_BAD_INPUT, "the transcript serves domains up to 2^%u, the circuit needs 2^%u", L.log, logn);
  const uint32_t n = 1u << logn, n_t1 = 2 * n - 1;
  if (circ.n_constraints > n || circ.challenge_wire >= W || circ.n_public > W) return fail(SPP_ERR_FORMAT, "%s is not a consistent circuit", circuit_path);
  for (uint32_t w : circ.committed)
    if (w >= W) return fail(SPP_ERR_FORMAT, "%s is not a consistent circuit", circuit_path);

  // the coefficient table in signed form, and the matrices as column entries:
  //   G1 columns [A_j | B_j | K_j] over the bases [L | alpha L | beta L]: K_j takes A's terms on beta L, B's on alpha L, C's on L
  //   G2 columns [B_j] over the bases L in G2
  const uint32_t ncoef = (uint32_t)circ.coeffs.size();
  std::vector<uint32_t> mags((size_t)8 * ncoef), meta(ncoef);
  for (uint32_t i = 0; i < ncoef; i++) {
    uint32_t c[8];
    circ.coeffs[i].to_canonical(c);
    meta[i] = pt_signed_coeff(c, &mags[(size_t)8 * i]);
  }
  std::vector<ColEntry> e1, e2;
  {
    const Sparse* M[3] = {&circ.A, &circ.B, &circ.C};
    for (int m = 0; m < 3; m++) {
      if (M[m]->rows() < circ.n_constraints) return fail(SPP_ERR_FORMAT, "%s is not a consistent circuit", circuit_path);
      for (uint32_t k = 0; k < circ.n_constraints; k++)
        for (uint32_t i = M[m]->rowptr[k]; i < M[m]->rowptr[k + 1]; i++) {
          const Term& t = M[m]->terms[i];
          if (t.wire >= W) return fail(SPP_ERR_FORMAT, "%s names a wire out of range", circuit_path);
          if (m < 2) e1.push_back({(uint32_t)m * W + t.wire, k, t.coeff});
          if (m == 1) e2.push_back({t.wire, k, t.coeff});
          e1.push_back({2 * W + t.wire, (m == 0 ? 2 * n : m == 1 ? n : 0) + k, t.coeff});
        }
    }
  }

  // the transcript's points this circuit uses: T1[0 .. 2n - 1), T2, A1, B1 [0 .. n) and beta2, every one checked before it is used
  std::vector<uint8_t> g1_raw((size_t)(n_t1 + 2 * n) * 64);
  memcpy(g1_raw.data(), pt.data() + L.t1, (size_t)n_t1 * 64);
  memcpy(g1_raw.data() + (size_t)n_t1 * 64, pt.data() + L.a1, (size_t)n * 64);
  memcpy(g1_raw.data() + (size_t)(n_t1 + n) * 64, pt.data() + L.b1, (size_t)n * 64);
  KeyPoints kp{};
  if (!g2_raw_valid(pt.data() + L.beta2, &kp.beta2)) return fail(SPP_ERR_FORMAT, "%s: beta2 is not a point of the group", ptau_path);
  std::vector<G1Affine> cols1, Z(n - 1);
  std::vector<G2Affine> cols2;
  {
    std::lock_guard<std::mutex> lk(ctx->mu);
    HIP_TRY(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    DevBuf d_g1, d_g2;
    std::vector<uint32_t> f1, f2;
    if (int e = decode_raw<Fq>(st, g1_raw.data(), n_t1 + 2 * n, d_g1, f1)) return e;
    if (int e = decode_raw<Fq2>(st, pt.data() + L.t2, n, d_g2, f2)) return e;
    for (size_t i = 0; i < f1.size(); i++)
      if (f1[i] != SC_POINT_OK) return fail(SPP_ERR_FORMAT, "%s: G1 point %zu (T1 | A1 | B1) is not a point of the curve", ptau_path, i);
    for (size_t i = 0; i < f2.size(); i++)
      if (f2[i] != SC_POINT_OK) return fail(SPP_ERR_FORMAT, "%s: T2 point %zu is not a point of the twist", ptau_path, i);
    if (!g2_all_in_subgroup(pt.data() + L.t2, n)) return fail(SPP_ERR_FORMAT, "%s: a T2 point is outside the order-r subgroup", ptau_path);

    // Lagrange points: three transforms in G1 (over T1[0 .. n), A1, B1) in one batch, one in G2
    const G1Affine* T1 = d_g1.as<G1Affine>();
    DevBuf d_in1, d_l1, d_l2, d_z, d_mags, d_meta;
    HIP_TRY(d_in1.alloc((size_t)3 * n * sizeof(G1Affine)));
    HIP_TRY(hipMemcpyAsync(d_in1.p, T1, (size_t)n * sizeof(G1Affine), hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_in1.as<G1Affine>() + n, T1 + n_t1, (size_t)2 * n * sizeof(G1Affine), hipMemcpyDeviceToDevice, st));
    HIP_TRY(d_l1.alloc((size_t)3 * n * sizeof(G1Affine)));
    HIP_TRY(d_l2.alloc((size_t)n * sizeof(G2Affine)));
    if (int e = intt_on_device<Fq>(st, d_in1.as<G1Affine>(), logn, 3, d_l1.as<G1Affine>())) return e;
    if (int e = intt_on_device<Fq2>(st, d_g2.as<G2Affine>(), logn, 1, d_l2.as<G2Affine>())) return e;
    // Z_i = T1_{i+n} - T1_i
    HIP_TRY(d_z.alloc((size_t)n * sizeof(G1Affine)));
    launch_g1_shifted_diff(st, T1, n, n - 1, d_z.as<G1Affine>());
    HIP_TRY(hipGetLastError());
    if (n > 1) HIP_TRY(hipMemcpyAsync(Z.data(), d_z.p, (size_t)(n - 1) * sizeof(G1Affine), hipMemcpyDeviceToHost, st));
    // the column gathers
    UP(d_mags, mags.data(), mags.size() * sizeof(uint32_t));
    UP(d_meta, meta.data(), meta.size() * sizeof(uint32_t));
    if (int e = gather_on_device<Fq>(st, d_l1.as<G1Affine>(), 3 * n, 3 * W, e1, d_mags.as<uint32_t>(), d_meta.as<uint32_t>(), ncoef, cols1)) return e;
    if (int e = gather_on_device<Fq2>(st, d_l2.as<G2Affine>(), n, W, e2, d_mags.as<uint32_t>(), d_meta.as<uint32_t>(), ncoef, cols2)) return e;
  }

  // gamma = delta = sigma = rho = 1: the generators stand where their powers would, CS = CB, the commitment key is (G2, -G2)
  kp.A = cols1.data();
  kp.B1 = cols1.data() + W;
  kp.K = kp.S = cols1.data() + 2 * (size_t)W;
  kp.B2 = cols2.data();
  kp.Z = Z.data();
  sc_decode_point(pt.data() + L.a1, &kp.alpha1);
  sc_decode_point(pt.data() + L.b1, &kp.beta1);
  kp.delta1 = g1_generator();
  kp.gamma2 = kp.delta2 = kp.ped_g = g2_generator();
  kp.ped_gs = kp.ped_g.neg();
  std::vector<uint8_t> o, v;
  key_files(circ, wire_classes(circ), kp, o, v);
  if (!write_file(pk_path, o)) return fail(SPP_ERR_IO, "cannot write %s", pk_path);
  if (!write_file(vk_path, v)) return fail(SPP_ERR_IO, "cannot write %s", vk_path);
  return SPP_OK;
}
