// libspp C ABI, what comes before a circuit is loaded: circuit construction (host only) and the trusted setup on the GPU.
#include "spp_internal.hpp"
#include "sppk_write.hpp"

// -----------------------------------------------------------------------------------------------------
// circuit construction (host only)
// -----------------------------------------------------------------------------------------------------
extern "C" int spp_circuit_build(int circuit_id, const uint32_t* aux, const char* out_path, uint32_t* n_constraints) {
  if (!out_path) return fail(SPP_ERR_BAD_INPUT, "out_path is NULL");
  Circuit c;
  if (circuit_id == SPP_CIRCUIT_WITHDRAW) {
    c = build_withdraw_circuit(true);
  } else if (circuit_id == SPP_CIRCUIT_WITHDRAW_REFSHAPE) {
    c = build_withdraw_circuit(true, 12452);
  } else if (circuit_id == SPP_CIRCUIT_WITHDRAW_DEPTH20) {
    c = build_withdraw_circuit(true, 0, 20);
  } else if (circuit_id == SPP_CIRCUIT_AUDIT) {
    if (!aux) return fail(SPP_ERR_BAD_INPUT, "audit circuit needs the RLWE public key (aux)");
    c = build_audit_circuit(aux, aux + 1024, true);
  } else if (circuit_id == SPP_CIRCUIT_DEPOSIT) {
    c = build_deposit_circuit(true, SPP_TREE_DEPTH);
  } else {
    return fail(SPP_ERR_BAD_INPUT, "unknown circuit id %d", circuit_id);
  }
  if (n_constraints) *n_constraints = c.n_constraints;
  if (!c.save(out_path)) return fail(SPP_ERR_IO, "cannot write %s", out_path);
  return SPP_OK;
}

// `sunspot compile <acir>` for a nargo-compiled program: blob = spp/acir.py to_blob() (the decoded opcode list)
extern "C" int spp_circuit_build_acir(const uint8_t* blob, size_t blob_len, int circuit_id, const char* out_path, uint32_t* n_constraints) {
  if (!blob || !out_path) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  Circuit c;
  std::string err;
  if (!build_acir_circuit(blob, blob_len, circuit_id > 0 ? (uint32_t)circuit_id : CIRCUIT_ACIR, &c, &err))
    return fail(SPP_ERR_FORMAT, "ACIR program not supported: %s", err.c_str());
  if (n_constraints) *n_constraints = c.n_constraints;
  if (!c.save(out_path)) return fail(SPP_ERR_IO, "cannot write %s", out_path);
  return SPP_OK;
}

// -----------------------------------------------------------------------------------------------------
// setup on the GPU
// -----------------------------------------------------------------------------------------------------
extern "C" int spp_setup(spp_ctx* ctx, const char* circuit_path, const uint8_t seed[32], const char* pk_path, const char* vk_path) {
  if (!ctx || !circuit_path || !seed || !pk_path || !vk_path) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  Circuit circ;
  if (!circ.load(circuit_path)) return fail(SPP_ERR_IO, "cannot read circuit %s", circuit_path);
  // toxic waste = hash_to_fr(seed, "spp-groth16-setup-v1", 7)
  Fr tox[7];
  {
    const char* dst = "spp-groth16-setup-v1";
    uint8_t u[7 * 48];
    expand_message_xmd(seed, 32, (const uint8_t*)dst, strlen(dst), u, sizeof u);
    for (int i = 0; i < 7; i++) {
      uint32_t w[12];
      for (int k = 0; k < 12; k++) {
        const uint8_t* q = u + 48 * i + 4 * k;
        w[k] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | q[3];
      }
      tox[i] = fr_from_wide48(w);
    }
  }
  const Fr tau = tox[0], alpha = tox[1], beta = tox[2], gamma = tox[3], delta = tox[4], sigma = tox[5], rho = tox[6];
  const uint32_t logn = circ.domain_log, n = 1u << logn, W = circ.n_wires;
  // Lagrange basis at tau
  std::vector<Fr> L(n), den(n), pre(n);
  {
    Fr omega = fr_root_of_unity(logn);
    Fr zt = tau.pow_u64(n) - Fr::one();
    Fr scale = zt * Fr::from_u64(n).inv();
    Fr wk = Fr::one(), acc = Fr::one();
    for (uint32_t k = 0; k < n; k++) {
      den[k] = tau - wk;
      pre[k] = acc;
      acc = acc * den[k];
      L[k] = wk;
      wk = wk * omega;
    }
    Fr ia = acc.inv();
    for (uint32_t k = n; k-- > 0;) {
      Fr di = ia * pre[k];
      ia = ia * den[k];
      L[k] = L[k] * di * scale;
    }
  }
  std::vector<Fr> aw(W, Fr::zero()), bw(W, Fr::zero()), cw(W, Fr::zero());
  {
    const Sparse* M[3] = {&circ.A, &circ.B, &circ.C};
    std::vector<Fr>* O[3] = {&aw, &bw, &cw};
    for (int m = 0; m < 3; m++)
      for (uint32_t k = 0; k < circ.n_constraints; k++)
        for (uint32_t i = M[m]->rowptr[k]; i < M[m]->rowptr[k + 1]; i++) {
          const Term& t = M[m]->terms[i];
          (*O[m])[t.wire] = (*O[m])[t.wire] + circ.coeffs[t.coeff] * L[k];
        }
  }
  const std::vector<uint8_t> cls = wire_classes(circ);
  const Fr gi = gamma.inv(), di = delta.inv();
  // scalar vectors, one fixed-base multiplication each:
  //   G1: [A(W) | B1(W) | K(W) | S(W) | Z(n-1) | alpha beta delta]    G2: [B2(W) | beta gamma delta rho -rho*sigma]
  std::vector<Fr> s1, s2;
  s1.reserve((size_t)4 * W + n + 3);
  for (uint32_t j = 0; j < W; j++) s1.push_back(aw[j]);
  for (uint32_t j = 0; j < W; j++) s1.push_back(bw[j]);
  std::vector<Fr> kk(W);
  for (uint32_t j = 0; j < W; j++) kk[j] = (beta * aw[j] + alpha * bw[j] + cw[j]) * (cls[j] ? gi : di);
  for (uint32_t j = 0; j < W; j++) s1.push_back(kk[j]);
  for (uint32_t j = 0; j < W; j++) s1.push_back(cls[j] == 2 ? kk[j] * sigma : Fr::zero());
  {
    Fr zt = tau.pow_u64(n) - Fr::one();
    Fr pw = zt * di;
    for (uint32_t i = 0; i + 1 < n; i++) {
      s1.push_back(pw);
      pw = pw * tau;
    }
  }
  s1.push_back(alpha); s1.push_back(beta); s1.push_back(delta);
  for (uint32_t j = 0; j < W; j++) s2.push_back(bw[j]);
  s2.push_back(beta); s2.push_back(gamma); s2.push_back(delta); s2.push_back(rho); s2.push_back((rho * sigma).neg());

  // generator tables (c = 8) and the batched fixed-base multiplications on the GPU
  const uint32_t cb = 8;
  G1Affine g1{Fq::from_u64(1), Fq::from_u64(2)};
  auto fq_dec = [](const char* dec) {
    Fq acc = Fq::zero(), ten = Fq::from_u64(10);
    for (const char* ch = dec; *ch; ch++) acc = acc * ten + Fq::from_u64((uint64_t)(*ch - '0'));
    return acc;
  };
  G2Affine g2;
  g2.x.c0 = fq_dec("10857046999023057135944570762232829481370756359578518086990519993285655852781");
  g2.x.c1 = fq_dec("11559732032986387107991004021392285783925812861821192530917403151452391805634");
  g2.y.c0 = fq_dec("8495653923123431417604973247489272438418190587263600148770280649306958101930");
  g2.y.c1 = fq_dec("4082367875863433681332203403145435568316851327593401208105741076214120093531");
  DevBuf t1, t2, d_s1, d_s2, o1, o2;   // released on every return path
  if (int e = build_generator_table<Fq>(st, g1, cb, t1)) return e;
  if (int e = build_generator_table<Fq2>(st, g2, cb, t2)) return e;
  HIP_TRY(d_s1.alloc(sizeof(Fr) * s1.size())); HIP_TRY(d_s2.alloc(sizeof(Fr) * s2.size()));
  HIP_TRY(o1.alloc(sizeof(G1Affine) * s1.size())); HIP_TRY(o2.alloc(sizeof(G2Affine) * s2.size()));
  HIP_TRY(hipMemcpyAsync(d_s1.p, s1.data(), sizeof(Fr) * s1.size(), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(d_s2.p, s2.data(), sizeof(Fr) * s2.size(), hipMemcpyHostToDevice, st));
  launch_fixed_base_mul<Fq>(st, t1.as<G1Affine>(), cb, d_s1.as<Fr>(), (uint32_t)s1.size(), o1.as<G1Affine>());
  launch_fixed_base_mul<Fq2>(st, t2.as<G2Affine>(), cb, d_s2.as<Fr>(), (uint32_t)s2.size(), o2.as<G2Affine>());
  std::vector<G1Affine> p1(s1.size());
  std::vector<G2Affine> p2(s2.size());
  HIP_TRY(hipMemcpyAsync(p1.data(), o1.p, sizeof(G1Affine) * p1.size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(p2.data(), o2.p, sizeof(G2Affine) * p2.size(), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());

  const G1Affine* pA = p1.data();
  const G1Affine* pB1 = pA + W;
  const G1Affine* pK = pB1 + W;
  const G1Affine* pS = pK + W;
  const G1Affine* pZ = pS + W;
  const G1Affine* pC = pZ + (n - 1);
  const G2Affine* pB2 = p2.data();
  const G2Affine* pC2 = pB2 + W;

  KeyPoints kp{pA, pB1, pK, pS, pB2, pZ, pC[0], pC[1], pC[2], pC2[0], pC2[1], pC2[2], pC2[3], pC2[4]};
  std::vector<uint8_t> o, v;
  key_files(circ, cls, kp, o, v);
  if (!write_file(pk_path, o)) return fail(SPP_ERR_IO, "cannot write %s", pk_path);
  if (!write_file(vk_path, v)) return fail(SPP_ERR_IO, "cannot write %s", vk_path);
  return SPP_OK;
}
