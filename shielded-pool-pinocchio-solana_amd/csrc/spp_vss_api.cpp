// libspp C ABI, the auditors' key without a dealer: the Pedersen sharing each auditor makes of its own part of the key, the
// receiver's check of every dealer's commitments and the sum that is its share (vss.hpp has the method, kernels_vss.hip the
// kernels, include/spp.h the protocol).  Everything that held a secret, a blind, a sharing coefficient or a sub-share is wiped.
#include "spp_internal.hpp"
#include "secret_buffers.hpp"
#include "vss.hpp"

namespace {
const size_t VSS_MAX_VALUES = (size_t)1 << 20;

// the window table of G and H, once per context: 64 window bases from the host, their 255 multiples on the device.  ctx->mu held
int ensure_vss_table(spp_ctx* ctx) {
  if (ctx->vss_table) return 0;
  std::vector<G1Affine> wb(2 * VSS_WINDOWS);
  vss_window_bases(wb.data());
  hipStream_t st = ctx->stream;
  DevBuf dw;
  UP(dw, wb.data(), sizeof(G1Affine) * wb.size());
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, sizeof(G1Affine) * VSS_TABLE_POINTS));
  ctx->owned.push_back(p);
  launch_vss_table(st, dw.as<G1Affine>(), (G1Affine*)p);
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  ctx->vss_table = (G1Affine*)p;
  return 0;
}

int check_elements(const char* what, const uint8_t* v, size_t count) {
  for (size_t i = 0; i < count; i++)
    if (!be_is_canonical<FrParams>(v + 32 * i)) return fail(SPP_ERR_BAD_INPUT, "%s %zu is not a canonical field element", what, i);
  return SPP_OK;
}
}  // namespace

extern "C" int spp_vss_generators(uint8_t g[64], uint8_t h[64]) {
  if (!g || !h) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  g1_to_raw(vss_generator_g(), g);
  g1_to_raw(vss_generator_h(), h);
  return SPP_OK;
}

extern "C" int spp_dkg_a_from_seed(const uint8_t seed[32], uint32_t a[1024]) {
  if (!seed || !a) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  vss_a_from_seed(seed, a);
  return SPP_OK;
}

extern "C" int spp_vss_deal_timed(spp_ctx* ctx, uint32_t t, uint32_t m, const uint32_t* xs, size_t n, const uint8_t* secrets_be,
                                  const uint8_t* blinds_be, const uint8_t* coeffs_be, const uint8_t* coeffs_blind_be, uint8_t* ys,
                                  uint8_t* ys_blind, uint8_t* commitments, uint8_t* blinds_out, float ms[2]) {
  if (!ctx || !secrets_be || !ys || !ys_blind || !commitments) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (t == 0 || t > 64) return fail(SPP_ERR_BAD_INPUT, "threshold %u is not in [1, 64]", t);
  if (m < t || m > 255) return fail(SPP_ERR_BAD_INPUT, "%u shares: need between the threshold %u and 255", m, t);
  if (xs)
    for (uint32_t j = 0; j < m; j++) {
      if (xs[j] == 0) return fail(SPP_ERR_BAD_INPUT, "xs[%u] is 0: that share would be the secret", j);
      for (uint32_t k = 0; k < j; k++)
        if (xs[k] == xs[j]) return fail(SPP_ERR_BAD_INPUT, "xs[%u] repeats xs[%u] = %u", j, k, xs[j]);
    }
  if (n > VSS_MAX_VALUES) return fail(SPP_ERR_BAD_INPUT, "n %zu: at most 2^20 values in one call", n);
  if (ms) ms[0] = ms[1] = 0;
  if (n == 0) return SPP_OK;
  const size_t ncoef = (size_t)(t - 1) * n;
  if (int rc = check_elements("secret", secrets_be, n)) return rc;
  if (blinds_be)
    if (int rc = check_elements("blind", blinds_be, n)) return rc;
  if (coeffs_be)
    if (int rc = check_elements("coefficient", coeffs_be, ncoef)) return rc;
  if (coeffs_blind_be)
    if (int rc = check_elements("blinding coefficient", coeffs_blind_be, ncoef)) return rc;
  // what the caller does not bring, from the OS: [blinds n | coeffs ncoef | coeffs_blind ncoef], each part only when missing
  WipedBytes drawn;
  {
    const size_t need = (blinds_be ? 0 : n) + (coeffs_be ? 0 : ncoef) + (coeffs_blind_be ? 0 : ncoef);
    drawn.v.resize(need * 32);
    OsRandom rnd;
    if (int rc = draw_field_elements(rnd, drawn.v.data(), need)) return rc;
    const uint8_t* at = drawn.v.data();
    if (!blinds_be) { blinds_be = at; at += n * 32; }
    if (!coeffs_be) { coeffs_be = at; at += ncoef * 32; }
    if (!coeffs_blind_be) coeffs_blind_be = at;
  }
  std::vector<Fr> x(m);
  for (uint32_t j = 0; j < m; j++) x[j] = Fr::from_u64(xs ? xs[j] : j + 1);
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (int rc = ensure_vss_table(ctx)) return rc;
  struct Events {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    ~Events() { for (hipEvent_t v : e) if (v) (void)hipEventDestroy(v); }
  } ev;
  if (ms)
    for (hipEvent_t& v : ev.e) HIP_TRY(hipEventCreate(&v));
  const size_t nys = (size_t)m * n * 32;
  WipedDevBuf ds, db, dc, dcb, dy, dyb;
  DevBuf dx, dcm;
  UP(dx, x.data(), sizeof(Fr) * m);
  UP_SECRET(ds, secrets_be, n * 32);
  UP_SECRET(db, blinds_be, n * 32);
  UP_SECRET(dc, coeffs_be, ncoef * 32);
  UP_SECRET(dcb, coeffs_blind_be, ncoef * 32);
  dy.bytes = dyb.bytes = nys;
  dy.st = dyb.st = st;
  HIP_TRY(dy.alloc(nys));
  HIP_TRY(dyb.alloc(nys));
  HIP_TRY(dcm.alloc((size_t)t * n * 64));
  if (ms) HIP_TRY(hipEventRecord(ev.e[0], st));
  launch_shamir_split(st, dx.as<Fr>(), ds.as<uint8_t>(), dc.as<uint8_t>(), t, m, (uint32_t)n, dy.as<uint8_t>());
  launch_shamir_split(st, dx.as<Fr>(), db.as<uint8_t>(), dcb.as<uint8_t>(), t, m, (uint32_t)n, dyb.as<uint8_t>());
  if (ms) HIP_TRY(hipEventRecord(ev.e[1], st));
  launch_vss_commit(st, ctx->vss_table, ds.as<uint8_t>(), dc.as<uint8_t>(), db.as<uint8_t>(), dcb.as<uint8_t>(), t, (uint32_t)n, dcm.as<uint8_t>());
  if (ms) HIP_TRY(hipEventRecord(ev.e[2], st));
  HIP_TRY(hipMemcpyAsync(ys, dy.p, nys, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(ys_blind, dyb.p, nys, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(commitments, dcm.p, (size_t)t * n * 64, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  if (ms) {
    HIP_TRY(hipEventElapsedTime(&ms[0], ev.e[0], ev.e[1]));
    HIP_TRY(hipEventElapsedTime(&ms[1], ev.e[1], ev.e[2]));
  }
  if (blinds_out) memcpy(blinds_out, blinds_be, n * 32);
  return SPP_OK;
}
extern "C" int spp_vss_deal(spp_ctx* ctx, uint32_t t, uint32_t m, const uint32_t* xs, size_t n, const uint8_t* secrets_be,
                            const uint8_t* blinds_be, const uint8_t* coeffs_be, const uint8_t* coeffs_blind_be, uint8_t* ys, uint8_t* ys_blind,
                            uint8_t* commitments, uint8_t* blinds_out) {
  return spp_vss_deal_timed(ctx, t, m, xs, n, secrets_be, blinds_be, coeffs_be, coeffs_blind_be, ys, ys_blind, commitments, blinds_out, nullptr);
}

extern "C" int spp_vss_receive(spp_ctx* ctx, uint32_t t, uint32_t x, uint32_t dealers, size_t n, const uint8_t* commitments, const uint8_t* ys,
                               const uint8_t* ys_blind, const uint8_t* zero_blinds, const uint8_t* base_be, uint32_t* flags,
                               uint8_t* share_out, size_t* bad) {
  if (!ctx || !commitments || !ys || !ys_blind || !flags || !bad) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (t == 0 || t > 64) return fail(SPP_ERR_BAD_INPUT, "threshold %u is not in [1, 64]", t);
  if (x == 0) return fail(SPP_ERR_BAD_INPUT, "x is 0: that share would be the secret");
  if (dealers == 0 || dealers > 255) return fail(SPP_ERR_BAD_INPUT, "%u dealers: need between 1 and 255", dealers);
  if (n > VSS_MAX_VALUES) return fail(SPP_ERR_BAD_INPUT, "n %zu: at most 2^20 values in one call", n);
  if (n == 0) {
    *bad = 0;
    return SPP_OK;
  }
  const size_t lanes = (size_t)dealers * n;
  if (int rc = check_elements("sub-share", ys, lanes)) return rc;
  if (int rc = check_elements("sub-share blind", ys_blind, lanes)) return rc;
  if (zero_blinds)
    if (int rc = check_elements("published blind", zero_blinds, lanes)) return rc;
  if (base_be)
    if (int rc = check_elements("base share value", base_be, n)) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (int rc = ensure_vss_table(ctx)) return rc;
  WipedDevBuf dy, dyb, dbase, dout;
  DevBuf dcm, dz, df;
  UP(dcm, commitments, lanes * t * 64);
  UP_SECRET(dy, ys, lanes * 32);
  UP_SECRET(dyb, ys_blind, lanes * 32);
  if (zero_blinds) UP(dz, zero_blinds, lanes * 32);
  HIP_TRY(df.alloc(lanes * 4));
  launch_vss_check(st, ctx->vss_table, t, x, dealers, (uint32_t)n, dcm.as<uint8_t>(), dy.as<uint8_t>(), dyb.as<uint8_t>(),
                   zero_blinds ? dz.as<uint8_t>() : nullptr, df.as<uint32_t>());
  HIP_TRY(hipMemcpyAsync(flags, df.p, lanes * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  size_t nbad = 0;
  for (size_t i = 0; i < lanes; i++) nbad += flags[i] != 0;
  *bad = nbad;
  if (nbad || !share_out) return SPP_OK;
  if (base_be) UP_SECRET(dbase, base_be, n * 32);
  dout.bytes = n * 32;
  dout.st = st;
  HIP_TRY(dout.alloc(n * 32));
  launch_vss_sum(st, base_be ? dbase.as<uint8_t>() : nullptr, dy.as<uint8_t>(), dealers, (uint32_t)n, dout.as<uint8_t>());
  HIP_TRY(hipMemcpyAsync(share_out, dout.p, n * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}

// ---- the committee's commitments, and handing the key to a new committee (include/spp.h, the block after spp_vss_receive) ----
namespace {
int check_threshold(const char* what, uint32_t t) {
  if (t == 0 || t > 64) return fail(SPP_ERR_BAD_INPUT, "%s %u is not in [1, 64]", what, t);
  return SPP_OK;
}
int check_indices(const char* what, const uint32_t* xs, uint32_t count) {
  for (uint32_t j = 0; j < count; j++) {
    if (xs[j] == 0) return fail(SPP_ERR_BAD_INPUT, "%s[%u] is 0: that share would be the secret", what, j);
    for (uint32_t k = 0; k < j; k++)
      if (xs[k] == xs[j]) return fail(SPP_ERR_BAD_INPUT, "%s[%u] repeats %s[%u] = %u", what, j, what, k, xs[j]);
  }
  return SPP_OK;
}
// the caller's own earlier output (a base, a committee file): every entry a point, checked on the host before any device work
int check_points(const char* what, const uint8_t* raw, size_t count) {
  G1Affine p;
  for (size_t i = 0; i < count; i++)
    if (sc_decode_point(raw + 64 * i, &p) == SC_POINT_BAD) return fail(SPP_ERR_BAD_INPUT, "%s %zu is not a curve point", what, i);
  return SPP_OK;
}
// weights as the scan reads them: 8 canonical words each, least significant first
void weight_words(const Fr* w, uint32_t count, std::vector<uint32_t>& out) {
  out.resize((size_t)8 * count);
  for (uint32_t d = 0; d < count; d++) w[d].to_canonical(out.data() + 8 * d);
}
}  // namespace

extern "C" int spp_vss_combine_commitments_timed(spp_ctx* ctx, uint32_t t, uint32_t dealers, size_t n, const uint8_t* commitments,
                                                 const uint8_t* weights_be, const uint8_t* base, uint8_t* out, uint32_t* flags, size_t* bad,
                                                 float* kernel_ms) {
  if (!ctx || !commitments || !out || !flags || !bad) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (int rc = check_threshold("threshold", t)) return rc;
  if (dealers == 0 || dealers > 255) return fail(SPP_ERR_BAD_INPUT, "%u dealers: need between 1 and 255", dealers);
  if (weights_be && dealers > VSS_LINCOMB_MAX) return fail(SPP_ERR_BAD_INPUT, "%u dealers: a weighted sum takes at most %u", dealers, VSS_LINCOMB_MAX);
  if (n > VSS_MAX_VALUES) return fail(SPP_ERR_BAD_INPUT, "n %zu: at most 2^20 values in one call", n);
  if (kernel_ms) *kernel_ms = 0;
  if (n == 0) {
    *bad = 0;
    return SPP_OK;
  }
  const size_t count = (size_t)t * n, inputs = count * dealers;
  std::vector<uint32_t> words;
  if (weights_be) {
    if (int rc = check_elements("weight", weights_be, dealers)) return rc;
    std::vector<Fr> w(dealers);
    for (uint32_t d = 0; d < dealers; d++) w[d] = Fr::from_bytes_be(weights_be + 32 * d);
    weight_words(w.data(), dealers, words);
  }
  if (base)
    if (int rc = check_points("base point", base, count)) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  struct Events {
    hipEvent_t e[2] = {nullptr, nullptr};
    ~Events() { for (hipEvent_t v : e) if (v) (void)hipEventDestroy(v); }
  } ev;
  if (kernel_ms)
    for (hipEvent_t& v : ev.e) HIP_TRY(hipEventCreate(&v));
  DevBuf draw, dpts, df, dw, dbraw, dbase, dbf, dout;
  UP(draw, commitments, inputs * 64);
  HIP_TRY(dpts.alloc(inputs * sizeof(G1Affine)));
  HIP_TRY(df.alloc(inputs * 4));
  if (weights_be) UP(dw, words.data(), words.size() * 4);
  if (base) {
    UP(dbraw, base, count * 64);
    HIP_TRY(dbase.alloc(count * sizeof(G1Affine)));
    HIP_TRY(dbf.alloc(count * 4));
  }
  HIP_TRY(dout.alloc(count * 64));
  if (kernel_ms) HIP_TRY(hipEventRecord(ev.e[0], st));
  launch_vss_decode(st, draw.as<uint8_t>(), inputs, dpts.as<G1Affine>(), df.as<uint32_t>());
  if (base) launch_vss_decode(st, dbraw.as<uint8_t>(), count, dbase.as<G1Affine>(), dbf.as<uint32_t>());
  // a non-point decodes as infinity: the sum below is then of no use, is computed all the same and is not copied out
  launch_vss_lincomb(st, dealers, weights_be ? dw.as<uint32_t>() : nullptr, dpts.as<G1Affine>(), base ? dbase.as<G1Affine>() : nullptr,
                     (uint32_t)count, dout.as<uint8_t>());
  if (kernel_ms) HIP_TRY(hipEventRecord(ev.e[1], st));
  HIP_TRY(hipMemcpyAsync(flags, df.p, inputs * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  if (kernel_ms) HIP_TRY(hipEventElapsedTime(kernel_ms, ev.e[0], ev.e[1]));
  size_t nbad = 0;
  for (size_t i = 0; i < inputs; i++) nbad += flags[i] != 0;
  *bad = nbad;
  if (nbad) return SPP_OK;
  HIP_TRY(hipMemcpyAsync(out, dout.p, count * 64, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return SPP_OK;
}
extern "C" int spp_vss_combine_commitments(spp_ctx* ctx, uint32_t t, uint32_t dealers, size_t n, const uint8_t* commitments,
                                           const uint8_t* weights_be, const uint8_t* base, uint8_t* out, uint32_t* flags, size_t* bad) {
  return spp_vss_combine_commitments_timed(ctx, t, dealers, n, commitments, weights_be, base, out, flags, bad, nullptr);
}

extern "C" int spp_vss_share_commitments(spp_ctx* ctx, uint32_t t, size_t n, const uint8_t* committee, uint32_t count, const uint32_t* xs,
                                         uint8_t* out) {
  if (!ctx || !committee || !xs || !out) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (int rc = check_threshold("threshold", t)) return rc;
  if (count == 0 || count > 255) return fail(SPP_ERR_BAD_INPUT, "%u indices: need between 1 and 255", count);
  if (int rc = check_indices("xs", xs, count)) return rc;
  if (n > VSS_MAX_VALUES) return fail(SPP_ERR_BAD_INPUT, "n %zu: at most 2^20 values in one call", n);
  if (n == 0) return SPP_OK;
  if (int rc = check_points("committee commitment", committee, (size_t)t * n)) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf dcm, dx, dout;
  UP(dcm, committee, (size_t)t * n * 64);
  UP(dx, xs, (size_t)count * 4);
  HIP_TRY(dout.alloc((size_t)count * n * 64));
  launch_vss_share_commit(st, t, dx.as<uint32_t>(), count, (uint32_t)n, dcm.as<uint8_t>(), dout.as<uint8_t>());
  HIP_TRY(hipMemcpyAsync(out, dout.p, (size_t)count * n * 64, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}

extern "C" int spp_vss_reshare_receive(spp_ctx* ctx, uint32_t t_old, const uint32_t* xs_old, uint32_t t_new, uint32_t x_new, size_t n,
                                       const uint8_t* committee, const uint8_t* commitments, const uint8_t* ys, const uint8_t* ys_blind,
                                       uint32_t* flags, uint8_t* share_out, uint8_t* blind_out, uint8_t* committee_out, size_t* bad) {
  if (!ctx || !xs_old || !committee || !commitments || !ys || !ys_blind || !flags || !share_out || !blind_out || !committee_out || !bad)
    return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (int rc = check_threshold("old threshold", t_old)) return rc;
  if (int rc = check_threshold("new threshold", t_new)) return rc;
  if (x_new == 0) return fail(SPP_ERR_BAD_INPUT, "x_new is 0: that share would be the secret");
  if (int rc = check_indices("xs_old", xs_old, t_old)) return rc;
  if (n > VSS_MAX_VALUES) return fail(SPP_ERR_BAD_INPUT, "n %zu: at most 2^20 values in one call", n);
  if (n == 0) {
    *bad = 0;
    return SPP_OK;
  }
  const size_t lanes = (size_t)t_old * n, count = (size_t)t_new * n, inputs = count * t_old;
  if (int rc = check_elements("sub-share", ys, lanes)) return rc;
  if (int rc = check_elements("sub-share blind", ys_blind, lanes)) return rc;
  if (int rc = check_points("committee commitment", committee, lanes)) return rc;
  std::vector<Fr> lambda(t_old);
  vss_lagrange_at_zero(xs_old, t_old, lambda.data());
  std::vector<uint32_t> words;
  weight_words(lambda.data(), t_old, words);
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (int rc = ensure_vss_table(ctx)) return rc;
  WipedDevBuf dy, dyb, dso, dbo;
  DevBuf dold, dcm, dx, df, dl, dw, dpts, dpf, dout;
  UP(dold, committee, lanes * 64);
  UP(dcm, commitments, inputs * 64);
  UP(dx, xs_old, (size_t)t_old * 4);
  UP_SECRET(dy, ys, lanes * 32);
  UP_SECRET(dyb, ys_blind, lanes * 32);
  HIP_TRY(df.alloc(lanes * 4));
  launch_vss_reshare_check(st, ctx->vss_table, t_old, dx.as<uint32_t>(), t_new, x_new, (uint32_t)n, dold.as<uint8_t>(), dcm.as<uint8_t>(),
                           dy.as<uint8_t>(), dyb.as<uint8_t>(), df.as<uint32_t>());
  HIP_TRY(hipMemcpyAsync(flags, df.p, lanes * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  size_t nbad = 0;
  for (size_t i = 0; i < lanes; i++) nbad += flags[i] != 0;
  *bad = nbad;
  if (nbad) return SPP_OK;
  // every check passed: the new share and blind (Lagrange-weighted sums of the sub-shares), the new committee's commitments
  UP(dl, lambda.data(), sizeof(Fr) * t_old);
  UP(dw, words.data(), words.size() * 4);
  dso.bytes = dbo.bytes = n * 32;
  dso.st = dbo.st = st;
  HIP_TRY(dso.alloc(n * 32));
  HIP_TRY(dbo.alloc(n * 32));
  HIP_TRY(dpts.alloc(inputs * sizeof(G1Affine)));
  HIP_TRY(dpf.alloc(inputs * 4));
  HIP_TRY(dout.alloc(count * 64));
  launch_vss_weighted_sum(st, dl.as<Fr>(), dy.as<uint8_t>(), t_old, (uint32_t)n, dso.as<uint8_t>());
  launch_vss_weighted_sum(st, dl.as<Fr>(), dyb.as<uint8_t>(), t_old, (uint32_t)n, dbo.as<uint8_t>());
  launch_vss_decode(st, dcm.as<uint8_t>(), inputs, dpts.as<G1Affine>(), dpf.as<uint32_t>());   // points all: the check above read every one
  launch_vss_lincomb(st, t_old, dw.as<uint32_t>(), dpts.as<G1Affine>(), nullptr, (uint32_t)count, dout.as<uint8_t>());
  HIP_TRY(hipMemcpyAsync(share_out, dso.p, n * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(blind_out, dbo.p, n * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(committee_out, dout.p, count * 64, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}
