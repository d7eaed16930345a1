// libspp C ABI, witness-input side: what the reference computes on the client before it can call the prover (RLWE encryption
// + quotient witnesses, Poseidon / Merkle / Grumpkin, the ct_commitment sponge, whole audit input rows) and the auditor side
// (Shamir reconstruction, BFV decryption), batched on the GPU.
#include "spp_internal.hpp"
#include "leaf_index.hpp"
#include "secret_buffers.hpp"

int spp_ensure_ctx_consts(spp_ctx* ctx) {
  if (ctx->consts_ready) return 0;
  auto flat = [](const PoseidonParams& pp) {
    std::vector<Fr> m;
    for (auto& row : pp.mds)
      for (auto& v : row) m.push_back(v);
    return m;
  };
  const PoseidonParams& p3 = poseidon_params(3);
  const PoseidonParams& p5 = poseidon_params(5);
  const Poseidon2Params& p2 = poseidon2_params();
  std::vector<Fr> mu(p2.mu, p2.mu + 4);
  Fr *a, *b, *c, *d, *f, *g;
  int e;
  auto canon = [](std::vector<Fr> v) {   // words < p: poseidon_permute29's value bounds rely on it
    for (auto& x : v) x = x.canonical();
    return v;
  };
  auto flat29 = [](const PoseidonParams& pp) {
    std::vector<uint32_t> m;
    for (auto& row : pp.mds)
      for (auto& v : row) {
        const F29<FrParams> x = F29<FrParams>::from_fp(v);     // v * 2^261, normalised, < 1.1 p
        for (int k = 0; k < 9; k++) m.push_back(x.l[k]);
      }
    return m;
  };
  uint32_t *m3, *m5;
  if ((e = ctx_upload(ctx, &a, canon(p3.rc))) || (e = ctx_upload(ctx, &b, flat(p3))) || (e = ctx_upload(ctx, &c, canon(p5.rc))) ||
      (e = ctx_upload(ctx, &d, flat(p5))) || (e = ctx_upload(ctx, &f, p2.rc)) || (e = ctx_upload(ctx, &g, mu)) ||
      (e = ctx_upload(ctx, &m3, flat29(p3))) || (e = ctx_upload(ctx, &m5, flat29(p5))))
    return e;
  ctx->hc = HashConsts{a, b, c, d, f, g, m3, m5};
  // Grumpkin window table T[j][d] = (d+1) * 16^j * G, j < 64, d < 16
  std::vector<GkAffine> tab(64 * 16);
  GkXYZZ base = GkXYZZ::from_affine(grumpkin_generator());
  for (int j = 0; j < 64; j++) {
    GkAffine ba = base.to_affine();
    GkXYZZ run = base;
    for (int dd = 0; dd < 16; dd++) {
      tab[j * 16 + dd] = run.to_affine();
      run.madd(ba);
    }
    base = GkXYZZ::from_affine(tab[j * 16 + 15]);
  }
  if ((e = ctx_upload(ctx, &ctx->gk_table, tab))) return e;
  ctx->consts_ready = true;
  return 0;
}
// twiddle / twist tables of the RLWE NTT kernel (32 KB) + the scratch that receives the transformed public key
int spp_ensure_rlwe(spp_ctx* ctx) {
  if (ctx->rlwe_ready) return 0;
  static RnHostTables h;   // 33 KB: not on the stack
  rn_build_tables(h);
  RlweDev& rd = ctx->rlwe;
  int e;
  for (int k = 0; k < 2; k++) {
    rd.tb.f[k] = h.f[k];
    rd.pk_scale[k] = h.pk_scale[k];
    int32_t *w0, *w1, *ps, *ips;
    if ((e = ctx_upload(ctx, &w0, std::vector<int32_t>(h.w[k][0], h.w[k][0] + 1024))) ||
        (e = ctx_upload(ctx, &w1, std::vector<int32_t>(h.w[k][1], h.w[k][1] + 1024))) ||
        (e = ctx_upload(ctx, &ps, std::vector<int32_t>(h.psi[k], h.psi[k] + 1024))) ||
        (e = ctx_upload(ctx, &ips, std::vector<int32_t>(h.ipsi[k], h.ipsi[k] + 1024))))
      return e;
    rd.tb.w[k][0] = w0; rd.tb.w[k][1] = w1; rd.tb.psi[k] = ps; rd.tb.ipsi[k] = ips;

  }
  void* p = nullptr;
  HIP_TRY(hipMalloc(&p, sizeof(RlwePkDev)));
  ctx->owned.push_back(p);
  rd.pk = (RlwePkDev*)p;
  ctx->rlwe_ready = true;
  return 0;
}

extern "C" int spp_rlwe_witness_batch(spp_ctx* ctx, const uint32_t* pk_a, const uint32_t* pk_b, size_t count, const int8_t* r,
                                      const int8_t* e1, const int8_t* e2, const uint8_t* msg, uint32_t* c0, uint32_t* c1, int32_t* k0,
                                      int32_t* k1, uint8_t* packed_be) {
  if (!ctx || !pk_a || !pk_b || !r || !e1 || !e2 || !msg || !c0 || !c1 || !k0 || !k1) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count == 0) return SPP_OK;
  for (int i = 0; i < 1024; i++)
    if (pk_a[i] >= 167772161u || pk_b[i] >= 167772161u) return fail(SPP_ERR_BAD_INPUT, "public key coefficient not in [0, q)");
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (int e = spp_ensure_rlwe(ctx)) return e;
  DevBuf da, db, dr, de1, de2, dm, dc0, dc1, dk0, dk1, dp;
  UP(da, pk_a, 4096); UP(db, pk_b, 4096);
  UP(dr, r, count * 1024); UP(de1, e1, count * 64); UP(de2, e2, count * 1024); UP(dm, msg, count * 64);
  HIP_TRY(dc0.alloc(count * 64 * 4)); HIP_TRY(dc1.alloc(count * 1024 * 4)); HIP_TRY(dk0.alloc(count * 64 * 4)); HIP_TRY(dk1.alloc(count * 1024 * 4));
  if (packed_be) HIP_TRY(dp.alloc(count * 157 * 32));
  launch_rlwe_witness(st, ctx->rlwe, da.as<uint32_t>(), db.as<uint32_t>(), dr.as<int8_t>(), de1.as<int8_t>(), de2.as<int8_t>(), dm.as<uint8_t>(),
                      dc0.as<uint32_t>(), dc1.as<uint32_t>(), dk0.as<int32_t>(), dk1.as<int32_t>(), packed_be ? dp.as<uint8_t>() : nullptr,
                      (uint32_t)count);
  HIP_TRY(hipMemcpyAsync(c0, dc0.p, count * 64 * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(c1, dc1.p, count * 1024 * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(k0, dk0.p, count * 64 * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(k1, dk1.p, count * 1024 * 4, hipMemcpyDeviceToHost, st));
  if (packed_be) HIP_TRY(hipMemcpyAsync(packed_be, dp.p, count * 157 * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}
// device-resident form (micro-benchmark: BASELINE.json configs[3]); all pointers are device pointers
extern "C" int spp_rlwe_witness_batch_device(spp_ctx* ctx, const void* d_pk_a, const void* d_pk_b, size_t count, const void* d_r,
                                             const void* d_e1, const void* d_e2, const void* d_msg, void* d_c0, void* d_c1, void* d_k0,
                                             void* d_k1, void* d_packed_be) {
  if (!ctx) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_rlwe(ctx)) return e;
  launch_rlwe_witness(ctx->stream, ctx->rlwe, (const uint32_t*)d_pk_a, (const uint32_t*)d_pk_b, (const int8_t*)d_r, (const int8_t*)d_e1,
                      (const int8_t*)d_e2, (const uint8_t*)d_msg, (uint32_t*)d_c0, (uint32_t*)d_c1, (int32_t*)d_k0, (int32_t*)d_k1,
                      (uint8_t*)d_packed_be, (uint32_t)count);
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}
extern "C" int spp_ctx_sync(spp_ctx* ctx) {
  if (!ctx) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  return SPP_OK;
}

extern "C" int spp_poseidon_hash_batch(spp_ctx* ctx, size_t count, int arity, const uint8_t* in, uint8_t* out) {
  if (!ctx || !in || !out) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (arity != 2 && arity != 4) return fail(SPP_ERR_BAD_INPUT, "arity must be 2 or 4");
  if (count == 0) return SPP_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  hipStream_t st = ctx->stream;
  DevBuf di, dout;
  UP(di, in, count * arity * 32);
  HIP_TRY(dout.alloc(count * 32));
  launch_poseidon_hash(st, ctx->hc, di.as<uint8_t>(), (uint32_t)arity, dout.as<uint8_t>(), (uint32_t)count);
  HIP_TRY(hipMemcpyAsync(out, dout.p, count * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}

extern "C" int spp_merkle_root_batch(spp_ctx* ctx, size_t count, uint32_t depth, const uint8_t* leaves, const uint64_t* indices,
                                     const uint8_t* siblings, uint8_t* roots) {
  if (!ctx || !leaves || !indices || !siblings || !roots) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (depth == 0 || depth > 64) return fail(SPP_ERR_BAD_INPUT, "depth out of range");
  if (count == 0) return SPP_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  hipStream_t st = ctx->stream;
  DevBuf dl, di, ds, dr;
  UP(dl, leaves, count * 32); UP(di, indices, count * 8); UP(ds, siblings, count * depth * 32);
  HIP_TRY(dr.alloc(count * 32));
  launch_merkle_path(st, ctx->hc, dl.as<uint8_t>(), di.as<uint64_t>(), ds.as<uint8_t>(), depth, dr.as<uint8_t>(), (uint32_t)count);
  HIP_TRY(hipMemcpyAsync(roots, dr.p, count * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}

// ShieldedPoolMerkleTree.getRoot + getProof (client/merkle.ts:165-221) for a tree of n_leaves inserted leaves
extern "C" int spp_merkle_build(spp_ctx* ctx, size_t n_leaves, uint32_t depth, const uint8_t* leaves, size_t n_queries,
                                const uint64_t* query_indices, uint8_t* siblings_out, uint8_t* root_out) {
  if (!ctx || !root_out || (n_leaves && !leaves) || (n_queries && (!query_indices || !siblings_out)))
    return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (depth == 0 || depth > 32 || n_leaves > ((size_t)1 << depth)) return fail(SPP_ERR_BAD_INPUT, "bad depth / too many leaves");
  for (size_t q = 0; q < n_queries; q++)
    if (query_indices[q] >= ((uint64_t)1 << depth)) return fail(SPP_ERR_BAD_INPUT, "query index out of range");
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  hipStream_t st = ctx->stream;
  // level sizes
  std::vector<size_t> cnt(depth + 1), off(depth + 2, 0);
  cnt[0] = n_leaves;
  for (uint32_t i = 0; i < depth; i++) cnt[i + 1] = (cnt[i] + 1) / 2;
  for (uint32_t i = 0; i <= depth; i++) off[i + 1] = off[i] + std::max<size_t>(cnt[i], 1);
  DevBuf dleaves, dnodes, ddef;
  UP(dleaves, leaves, n_leaves * 32);
  HIP_TRY(dnodes.alloc(off[depth + 1] * sizeof(Fr)));
  HIP_TRY(ddef.alloc((depth + 1) * sizeof(Fr)));
  Fr* nodes = dnodes.as<Fr>();
  launch_fr_from_be(st, dleaves.as<uint8_t>(), nodes, (uint32_t)n_leaves);
  std::vector<Fr> dflt(depth + 1);
  dflt[0] = Fr::zero();
  for (uint32_t i = 0; i < depth; i++) {
    // default hash of the next level: H(d_i, d_i) -- one lane, read back (depth <= 32 round trips at tree-build time)
    launch_merkle_level(st, ctx->hc, nullptr, 0, dflt[i], ddef.as<Fr>() + i + 1, 1);
    HIP_TRY(hipMemcpyAsync(&dflt[i + 1], ddef.as<Fr>() + i + 1, sizeof(Fr), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    launch_merkle_level(st, ctx->hc, nodes + off[i], (uint32_t)cnt[i], dflt[i], nodes + off[i + 1], (uint32_t)cnt[i + 1]);
  }
  std::vector<Fr> host(off[depth + 1]);
  HIP_TRY(hipMemcpyAsync(host.data(), nodes, host.size() * sizeof(Fr), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  Fr root = cnt[depth] ? host[off[depth]] : dflt[depth];
  root.to_bytes_be(root_out);
  for (size_t q = 0; q < n_queries; q++) {
    uint64_t idx = query_indices[q];
    for (uint32_t i = 0; i < depth; i++) {
      uint64_t sib = idx ^ 1;
      Fr v = sib < cnt[i] ? host[off[i] + sib] : dflt[i];
      v.to_bytes_be(siblings_out + (q * depth + i) * 32);
      idx >>= 1;
    }
  }
  return SPP_OK;
}

// -----------------------------------------------------------------------------------------------------
// incremental tree: ShieldedPoolMerkleTree (client/merkle.ts:146-222) with the levels kept in HBM.  insert() appends leaves and
// recomputes only the touched path(s): O(count + depth) hashes instead of the reference's O(2^depth) per getRoot / getProof.
// -----------------------------------------------------------------------------------------------------
// struct spp_merkle_tree: spp_internal.hpp (the withdraw-from-notes path of spp_prove.cpp reads its descriptor)
static size_t mt_level_cap(uint64_t cap_leaves, uint32_t l) { return (size_t)(cap_leaves >> l) + 1; }
static int mt_reserve(spp_merkle_tree* t, uint64_t want_leaves) {
  if (want_leaves <= t->cap_leaves) return 0;
  uint64_t cap = std::max<uint64_t>(t->cap_leaves ? t->cap_leaves : 1024, 1);
  while (cap < want_leaves) cap *= 2;
  cap = std::min<uint64_t>(cap, (uint64_t)1 << t->depth);
  hipStream_t st = t->ctx->stream;
  for (uint32_t l = 0; l <= t->depth; l++) {
    Fr* nw = nullptr;
    HIP_TRY(hipMalloc((void**)&nw, mt_level_cap(cap, l) * sizeof(Fr)));
    if (t->host.level[l]) {
      if (t->host.count[l]) HIP_TRY(hipMemcpyAsync(nw, t->host.level[l], t->host.count[l] * sizeof(Fr), hipMemcpyDeviceToDevice, st));
      HIP_TRY(hipStreamSynchronize(st));
      hipFree(t->host.level[l]);
    }
    t->host.level[l] = nw;
  }
  t->cap_leaves = cap;
  return 0;
}
static int mt_push_descriptor(spp_merkle_tree* t) {
  HIP_TRY(hipMemcpyAsync(t->dev, &t->host, sizeof(MerkleTreeDev), hipMemcpyHostToDevice, t->ctx->stream));
  return 0;
}
// append `count` leaves already written into level 0 at [n_leaves, n_leaves + count) (insert, deposit): the touched parents of
// every level are recomputed on the context's stream, then the descriptor is pushed; no synchronise
static int mt_append(spp_merkle_tree* t, uint64_t count) {
  spp_ctx* ctx = t->ctx;
  const uint64_t first = t->n_leaves, last = first + count - 1;
  t->n_leaves += count;
  t->host.count[0] = t->n_leaves;
  for (uint32_t l = 0; l < t->depth; l++) {
    const uint64_t p0 = first >> (l + 1), p1 = last >> (l + 1);
    launch_merkle_update(ctx->stream, ctx->hc, t->host.level[l], t->host.count[l], t->d_dflt + l, t->host.level[l + 1], p0,
                         (uint32_t)(p1 - p0 + 1));
    t->host.count[l + 1] = (t->host.count[l] + 1) / 2;
  }
  return mt_push_descriptor(t);
}
extern "C" int spp_merkle_tree_new(spp_ctx* ctx, uint32_t depth, spp_merkle_tree** out) {
  if (!ctx || !out) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (depth == 0 || depth > 32) return fail(SPP_ERR_BAD_INPUT, "depth must be 1..32");
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  spp_merkle_tree* t = new spp_merkle_tree();
  t->ctx = ctx;
  t->depth = depth;
  t->host.depth = depth;
  auto bail = [&](int e) { spp_merkle_tree_free(t); return e; };
  if (hipMalloc((void**)&t->dev, sizeof(MerkleTreeDev)) != hipSuccess || hipMalloc((void**)&t->d_dflt, 33 * sizeof(Fr)) != hipSuccess)
    return bail(fail(SPP_ERR_HIP, "hipMalloc"));
  launch_merkle_defaults(ctx->stream, ctx->hc, t->d_dflt, depth);
  if (hipMemcpyAsync(t->host.dflt, t->d_dflt, (depth + 1) * sizeof(Fr), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess)
    return bail(fail(SPP_ERR_HIP, "default hashes"));
  if (int e = mt_reserve(t, 1024)) return bail(e);
  if (int e = mt_push_descriptor(t)) return bail(e);
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  *out = t;
  return SPP_OK;
}
extern "C" void spp_merkle_tree_free(spp_merkle_tree* t) {
  if (!t) return;
  hipSetDevice(t->ctx->device);
  hipStreamSynchronize(t->ctx->stream);
  for (uint32_t l = 0; l <= 32; l++) if (t->host.level[l]) hipFree(t->host.level[l]);
  if (t->dev) hipFree(t->dev);
  if (t->d_dflt) hipFree(t->d_dflt);
  if (t->d_index) hipFree(t->d_index);
  if (t->d_frontier) hipFree(t->d_frontier);
  if (t->d_roots) hipFree(t->d_roots);
  if (t->d_root_index) hipFree(t->d_root_index);
  delete t;
}
extern "C" uint64_t spp_merkle_tree_size(const spp_merkle_tree* t) { return t ? t->n_leaves : 0; }
// insert(commitment) (merkle.ts:158-163) for `count` leaves at once; *first_index receives the index of the first one
extern "C" int spp_merkle_tree_insert(spp_merkle_tree* t, size_t count, const uint8_t* leaves, uint64_t* first_index) {
  if (!t || (count && !leaves)) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  for (size_t i = 0; i < count; i++)
    if (!be_is_canonical<FrParams>(leaves + 32 * i)) return fail(SPP_ERR_BAD_INPUT, "leaf %zu is not a canonical field element", i);
  spp_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);   // the size, the first index handed out and the "full" check are read under the lock:
                                             // two inserting threads must not get the same index
  if (first_index) *first_index = t->n_leaves;
  if (count == 0) return SPP_OK;
  if (count > ((uint64_t)1 << t->depth) - t->n_leaves) return fail(SPP_ERR_BAD_INPUT, "tree is full");
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (int e = mt_reserve(t, t->n_leaves + count)) return e;
  DevBuf dl;
  UP(dl, leaves, count * 32);
  launch_fr_from_be(st, dl.as<uint8_t>(), t->host.level[0] + t->n_leaves, (uint32_t)count);
  if (int e = mt_append(t, count)) return e;
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}
// calculateCommitment + insert + getRoot for every deposit (client/payroll-demo.ts:264-292) in one call: k_deposit_leaves writes
// level 0, the level update of insert runs once for the whole range, k_deposit_roots gives every deposit's prefix root
extern "C" int spp_merkle_tree_deposit(spp_merkle_tree* t, size_t count, const uint8_t* deposits, uint64_t* first_index,
                                       uint8_t* commitments, uint8_t* roots) {
  static const char* const field_name[3] = {"secret_key", "amount", "randomness"};
  if (!t || (count && !deposits)) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count > (1u << 24)) return fail(SPP_ERR_BAD_INPUT, "too many deposits in one call (%zu; at most 2^24)", count);
  for (size_t i = 0; i < count; i++) {
    const uint8_t* d = deposits + SPP_DEPOSIT_LEN * i;
    for (int f = 0; f < 3; f++)
      if (!be_is_canonical<FrParams>(d + 32 * f))
        return fail(SPP_ERR_BAD_INPUT, "deposit %zu: %s is not a canonical field element", i, field_name[f]);
    bool sk_zero = true, amount_u64 = true;
    for (int b = 0; b < 32; b++) sk_zero &= d[b] == 0;
    for (int b = 0; b < 24; b++) amount_u64 &= d[32 + b] == 0;
    if (sk_zero) return fail(SPP_ERR_BAD_INPUT, "deposit %zu: secret_key is 0", i);
    if (!amount_u64) return fail(SPP_ERR_BAD_INPUT, "deposit %zu: amount does not fit 64 bits", i);
  }
  spp_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);   // as insert: the first index handed out and the room check are read under the lock
  const uint64_t room = ((uint64_t)1 << t->depth) - t->n_leaves;
  if (count > room)
    return fail(SPP_ERR_BAD_INPUT, "deposit %llu: the tree is full (%llu of %llu leaves used)", (unsigned long long)room,
                (unsigned long long)t->n_leaves, (unsigned long long)1 << t->depth);
  if (first_index) *first_index = t->n_leaves;
  if (count == 0) return SPP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  hipStream_t st = ctx->stream;
  if (int e = mt_reserve(t, t->n_leaves + count)) return e;
  const uint64_t first = t->n_leaves;
  DevBuf dd, dout;
  UP(dd, deposits, count * SPP_DEPOSIT_LEN);
  launch_deposit_leaves(st, ctx->gk_table, ctx->hc, dd.as<uint8_t>(), t->host.level[0] + first, (uint32_t)count);
  if (int e = mt_append(t, count)) return e;
  if (commitments || roots) {
    HIP_TRY(dout.alloc(count * 64));
    uint8_t *d_com = dout.as<uint8_t>(), *d_roots = d_com + count * 32;
    launch_deposit_roots(st, ctx->hc, t->dev, first, (uint32_t)count, roots ? d_roots : nullptr, commitments ? d_com : nullptr);
    if (commitments) HIP_TRY(hipMemcpyAsync(commitments, d_com, count * 32, hipMemcpyDeviceToHost, st));
    if (roots) HIP_TRY(hipMemcpyAsync(roots, d_roots, count * 32, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}
// getRoot (merkle.ts:165-176): one 32-byte read
extern "C" int spp_merkle_tree_root(spp_merkle_tree* t, uint8_t root[32]) {
  if (!t || !root) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  std::lock_guard<std::mutex> lk(t->ctx->mu);
  HIP_TRY(hipSetDevice(t->ctx->device));
  Fr v = t->host.dflt[t->depth];
  if (t->n_leaves) HIP_TRY(hipMemcpy(&v, t->host.level[t->depth], sizeof(Fr), hipMemcpyDeviceToHost));
  v.to_bytes_be(root);
  return SPP_OK;
}
// getProof (merkle.ts:198-221) for n indices: siblings_out = n * depth * 32 B; no hashing, depth reads per query
extern "C" int spp_merkle_tree_proofs(spp_merkle_tree* t, size_t n, const uint64_t* indices, uint8_t* siblings_out) {
  if (!t || (n && (!indices || !siblings_out))) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (n == 0) return SPP_OK;
  if (n > (1u << 24)) return fail(SPP_ERR_BAD_INPUT, "too many queries in one call");
  for (size_t q = 0; q < n; q++)
    if (indices[q] >= ((uint64_t)1 << t->depth)) return fail(SPP_ERR_BAD_INPUT, "query index out of range");
  spp_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf di, dout;
  UP(di, indices, n * sizeof(uint64_t));
  HIP_TRY(dout.alloc(n * t->depth * 32));
  launch_merkle_gather(st, t->dev, t->depth, di.as<uint64_t>(), (uint32_t)n, dout.as<uint8_t>());
  HIP_TRY(hipMemcpyAsync(siblings_out, dout.p, n * t->depth * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}

// Withdraw rows from notes (client/payroll-demo.ts:323-340 for every recipient: identity, wa_commitment, nullifier, getRoot,
// getProof) against the tree as it stands: one k_withdraw_rows launch on the tree's stream.
int spp_check_notes(size_t count, const uint8_t* notes) {
  for (size_t i = 0; i < count; i++)
    for (int f = 0; f < 5; f++)
      if (!be_is_canonical<FrParams>(notes + SPP_NOTE_LEN * i + 32 * f))
        return fail(SPP_ERR_BAD_INPUT, "note %zu: field %d is not a canonical field element", i, f);
  return SPP_OK;
}
extern "C" int spp_withdraw_rows_from_tree(spp_merkle_tree* t, size_t count, const uint8_t* notes, uint8_t* rows) {
  if (!t || !notes || !rows) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count == 0) return SPP_OK;
  if (count > (1u << 24)) return fail(SPP_ERR_BAD_INPUT, "too many notes in one call");
  if (int e = spp_check_notes(count, notes)) return e;
  spp_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  hipStream_t st = ctx->stream;
  const size_t row_bytes = (size_t)(10 + t->depth) * 32;
  DevBuf dn, dr;
  UP(dn, notes, count * SPP_NOTE_LEN);
  HIP_TRY(dr.alloc(count * row_bytes));
  launch_withdraw_rows(st, ctx->gk_table, ctx->hc, t->dev, dn.as<uint8_t>(), dr.as<uint8_t>(), (uint32_t)count);
  HIP_TRY(hipMemcpyAsync(rows, dr.p, count * row_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}

// -----------------------------------------------------------------------------------------------------
// Wallet sync: from leaf values and from secrets back to positions (demo-frontend/app/lib/storage.ts:9-26,45-50,233-260: the
// DepositRecord / MerkleTreeState a wallet keeps, rebuilt instead of carried along).  The leaf index and its ordering argument are
// leaf_index.hpp; insert, deposit, root, proofs and the notes path never touch it.
// -----------------------------------------------------------------------------------------------------
static_assert(SPP_WALLET_RECORD_LEN == 160 && SPP_WALLET_IN_TREE == 1 && SPP_WALLET_SPENT == 2 && SPP_WALLET_AUDITED == 4 &&
                  SPP_WALLET_REPEATED == 8, "include/spp.h and kernels_witness.hip disagree");
static int mt_index_salt(uint64_t* salt) {
  if (const char* env = getenv("SPP_TREE_INDEX_SALT")) {
    char* end = nullptr;
    *salt = strtoull(env, &end, 16);
    if (end == env || *end) return fail(SPP_ERR_BAD_INPUT, "SPP_TREE_INDEX_SALT is not a hexadecimal number");
    return SPP_OK;
  }
  FILE* f = fopen("/dev/urandom", "rb");
  if (!f || fread(salt, 1, sizeof *salt, f) != sizeof *salt) {
    if (f) fclose(f);
    return fail(SPP_ERR_IO, "cannot read /dev/urandom");
  }
  fclose(f);
  return SPP_OK;
}
// Brings the index up to the tree (ctx->mu held, device set): leaves [indexed, n_leaves) are inserted in ONE launch on the context's
// stream; the caller's query is a later launch.  A table that would pass half full is allocated again at the larger size and every
// leaf reinserted.
// The same for any table of the tree over an Fr array (the leaf index over level 0, the root index over d_roots): entries
// [*indexed, n) of `values` are inserted, `want` slots wanted.
static int mt_table_sync(spp_merkle_tree* t, uint32_t** d_slots, uint32_t* slots, uint64_t* indexed, const Fr* values, uint64_t n, uint32_t want,
                         LeafIndex* ix) {
  if (!t->index_salted) {
    if (int e = mt_index_salt(&t->index_salt)) return e;
    t->index_salted = true;
  }
  hipStream_t st = t->ctx->stream;
  if (!*d_slots || want > *slots) {
    if (*d_slots) {
      HIP_TRY(hipStreamSynchronize(st));
      hipFree(*d_slots);
      *d_slots = nullptr;
    }
    *slots = 0;
    *indexed = 0;
    HIP_TRY(hipMalloc((void**)d_slots, (size_t)want * sizeof(uint32_t)));
    *slots = want;
    HIP_TRY(hipMemsetAsync(*d_slots, 0xFF, (size_t)want * sizeof(uint32_t), st));
  }
  *ix = LeafIndex{*d_slots, *slots - 1, t->index_salt};
  launch_leaf_index_insert(st, *ix, values, (uint32_t)*indexed, (uint32_t)(n - *indexed));
  *indexed = n;
  return SPP_OK;
}
static int mt_index_sync(spp_merkle_tree* t, LeafIndex* ix) {
  if (t->n_leaves > LEAF_INDEX_MAX_LEAVES)
    return fail(SPP_ERR_BAD_INPUT, "the tree has %llu leaves: the leaf index covers at most 2^30", (unsigned long long)t->n_leaves);
  return mt_table_sync(t, &t->d_index, &t->index_slots, &t->indexed, t->host.level[0], t->n_leaves, leaf_index_slots(t->n_leaves), ix);
}

extern "C" int spp_merkle_tree_find(spp_merkle_tree* t, size_t count, const uint8_t* leaves, const uint64_t* from, uint64_t* indices,
                                    uint32_t* matches) {
  if (!t || (count && (!leaves || !indices))) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count == 0) return SPP_OK;
  if (count > (1u << 24)) return fail(SPP_ERR_BAD_INPUT, "too many leaf values in one call (%zu; at most 2^24)", count);
  for (size_t i = 0; i < count; i++)
    if (!be_is_canonical<FrParams>(leaves + 32 * i)) return fail(SPP_ERR_BAD_INPUT, "leaf value %zu is not a canonical field element", i);
  spp_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  LeafIndex ix;
  if (int e = mt_index_sync(t, &ix)) return e;
  DevBuf dk, df, di, dm;
  UP(dk, leaves, count * 32);
  if (from) UP(df, from, count * sizeof(uint64_t));
  HIP_TRY(di.alloc(count * sizeof(uint64_t)));
  if (matches) HIP_TRY(dm.alloc(count * sizeof(uint32_t)));
  launch_leaf_find(st, ix, t->host.level[0], dk.as<uint8_t>(), from ? df.as<uint64_t>() : nullptr, di.as<uint64_t>(),
                   matches ? dm.as<uint32_t>() : nullptr, (uint32_t)count);
  HIP_TRY(hipMemcpyAsync(indices, di.p, count * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  if (matches) HIP_TRY(hipMemcpyAsync(matches, dm.p, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}

extern "C" int spp_wallet_sync(spp_merkle_tree* t, spp_pool* pool, size_t count, const uint8_t* deposits, const uint8_t* recipients,
                               uint64_t* indices, uint32_t* flags, uint8_t* records, uint8_t* notes) {
  static const char* const field_name[3] = {"secret_key", "amount", "randomness"};
  if (!t || (count && (!deposits || !indices || !flags))) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (notes && !recipients) return fail(SPP_ERR_BAD_INPUT, "notes are built from recipients: recipients is NULL");
  if (count > (1u << 24)) return fail(SPP_ERR_BAD_INPUT, "too many secrets in one call (%zu; at most 2^24)", count);
  for (size_t i = 0; i < count; i++) {
    const uint8_t* d = deposits + SPP_DEPOSIT_LEN * i;
    for (int f = 0; f < 3; f++)
      if (!be_is_canonical<FrParams>(d + 32 * f))
        return fail(SPP_ERR_BAD_INPUT, "secret %zu: %s is not a canonical field element", i, field_name[f]);
    bool sk_zero = true, amount_u64 = true;
    for (int b = 0; b < 32; b++) sk_zero &= d[b] == 0;
    for (int b = 0; b < 24; b++) amount_u64 &= d[32 + b] == 0;
    if (sk_zero) return fail(SPP_ERR_BAD_INPUT, "secret %zu: secret_key is 0", i);
    if (!amount_u64) return fail(SPP_ERR_BAD_INPUT, "secret %zu: amount does not fit 64 bits", i);
    if (recipients && !be_is_canonical<FrParams>(recipients + 32 * i))
      return fail(SPP_ERR_BAD_INPUT, "secret %zu: recipient is not a canonical field element", i);
  }
  spp_ctx* ctx = t->ctx;
  if (pool && spp_pool_view(pool, nullptr, nullptr) != ctx) return fail(SPP_ERR_BAD_INPUT, "the pool belongs to another spp_ctx than the tree");
  if (count == 0) return SPP_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  hipStream_t st = ctx->stream;
  PoolSet sets[2];
  uint64_t pool_salt = 0;
  if (pool) spp_pool_view(pool, sets, &pool_salt);
  LeafIndex ix;
  if (int e = mt_index_sync(t, &ix)) return e;
  DevBuf dd, dr, drec, di, df, dn;
  UP(dd, deposits, count * SPP_DEPOSIT_LEN);
  if (notes) UP(dr, recipients, count * 32);
  HIP_TRY(drec.alloc(count * SPP_WALLET_RECORD_LEN));
  HIP_TRY(di.alloc(count * sizeof(uint64_t)));
  HIP_TRY(df.alloc(count * sizeof(uint32_t)));
  if (notes) HIP_TRY(dn.alloc(count * SPP_NOTE_LEN));
  launch_wallet_sync(st, ctx->gk_table, ctx->hc, ix, t->dev, pool ? sets : nullptr, pool_salt, dd.as<uint8_t>(), notes ? dr.as<uint8_t>() : nullptr,
                     drec.as<uint8_t>(), di.as<uint64_t>(), df.as<uint32_t>(), notes ? dn.as<uint8_t>() : nullptr, (uint32_t)count);
  HIP_TRY(hipMemcpyAsync(indices, di.p, count * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(flags, df.p, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  if (records) HIP_TRY(hipMemcpyAsync(records, drec.p, count * SPP_WALLET_RECORD_LEN, hipMemcpyDeviceToHost, st));
  if (notes) HIP_TRY(hipMemcpyAsync(notes, dn.p, count * SPP_NOTE_LEN, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}

// -----------------------------------------------------------------------------------------------------
// The tree as of an earlier size: roots, paths and withdraw rows of the first `size` leaves, the roots of all sizes and the way
// back from a root word to its size (include/spp.h; the rule and why stored nodes can be reused is merkle_prefix.hpp).  Every as-of
// call enqueues k_merkle_frontier for its size and then the launch that reads t->d_frontier, both on the context's stream: a later
// call's frontier is stream-ordered behind the earlier call's reader.
// -----------------------------------------------------------------------------------------------------
int spp_tree_frontier_enqueue(spp_merkle_tree* t, uint64_t* size) {
  if (*size == SPP_TREE_SIZE_NOW) *size = t->n_leaves;
  if (*size > t->n_leaves)
    return fail(SPP_ERR_BAD_INPUT, "size %llu is larger than the tree, which has %llu leaves", (unsigned long long)*size,
                (unsigned long long)t->n_leaves);
  if (!t->d_frontier) HIP_TRY(hipMalloc((void**)&t->d_frontier, 33 * sizeof(Fr)));
  launch_merkle_frontier(t->ctx->stream, t->ctx->hc, t->dev, *size, t->d_frontier);
  return SPP_OK;
}
extern "C" int spp_merkle_tree_root_at(spp_merkle_tree* t, uint64_t size, uint8_t root[32]) {
  if (!t || !root) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (size == SPP_TREE_SIZE_NOW) return spp_merkle_tree_root(t, root);
  spp_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  hipStream_t st = ctx->stream;
  if (int e = spp_tree_frontier_enqueue(t, &size)) return e;
  Fr v;
  HIP_TRY(hipMemcpyAsync(&v, t->d_frontier + t->depth, sizeof(Fr), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  v.to_bytes_be(root);
  return SPP_OK;
}
extern "C" int spp_merkle_tree_proofs_at(spp_merkle_tree* t, uint64_t size, size_t n, const uint64_t* indices, uint8_t* siblings_out) {
  if (!t || (n && (!indices || !siblings_out))) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (size == SPP_TREE_SIZE_NOW) return spp_merkle_tree_proofs(t, n, indices, siblings_out);
  if (n > (1u << 24)) return fail(SPP_ERR_BAD_INPUT, "too many queries in one call");
  for (size_t q = 0; q < n; q++)
    if (indices[q] >= ((uint64_t)1 << t->depth)) return fail(SPP_ERR_BAD_INPUT, "query index out of range");
  spp_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (size > t->n_leaves) return spp_tree_frontier_enqueue(t, &size);   // the refusal, also for n == 0
  if (n == 0) return SPP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  hipStream_t st = ctx->stream;
  if (int e = spp_tree_frontier_enqueue(t, &size)) return e;
  DevBuf di, dout;
  UP(di, indices, n * sizeof(uint64_t));
  HIP_TRY(dout.alloc(n * t->depth * 32));
  launch_merkle_gather_at(st, t->dev, t->depth, size, t->d_frontier, di.as<uint64_t>(), (uint32_t)n, dout.as<uint8_t>());
  HIP_TRY(hipMemcpyAsync(siblings_out, dout.p, n * t->depth * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}
extern "C" int spp_withdraw_rows_from_tree_at(spp_merkle_tree* t, uint64_t size, size_t count, const uint8_t* notes, uint8_t* rows) {
  if (!t || !notes || !rows) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (size == SPP_TREE_SIZE_NOW) return spp_withdraw_rows_from_tree(t, count, notes, rows);
  if (count > (1u << 24)) return fail(SPP_ERR_BAD_INPUT, "too many notes in one call");
  if (int e = spp_check_notes(count, notes)) return e;
  spp_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (size > t->n_leaves) return spp_tree_frontier_enqueue(t, &size);   // the refusal, also for count == 0
  if (count == 0) return SPP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  hipStream_t st = ctx->stream;
  if (int e = spp_tree_frontier_enqueue(t, &size)) return e;
  const size_t row_bytes = (size_t)(10 + t->depth) * 32;
  DevBuf dn, dr;
  UP(dn, notes, count * SPP_NOTE_LEN);
  HIP_TRY(dr.alloc(count * row_bytes));
  launch_withdraw_rows_at(st, ctx->gk_table, ctx->hc, t->dev, size, t->d_frontier, dn.as<uint8_t>(), dr.as<uint8_t>(), (uint32_t)count);
  HIP_TRY(hipMemcpyAsync(rows, dr.p, count * row_bytes, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}

// R[0 .. n_leaves] resident (ctx->mu held, device set): the array grows by doubling, what was computed is copied, and only the
// sizes that came since are walked -- a prefix root never changes (merkle_prefix.hpp)
static int mt_roots_sync(spp_merkle_tree* t) {
  spp_ctx* ctx = t->ctx;
  hipStream_t st = ctx->stream;
  const uint64_t want = t->n_leaves + 1;
  if (want > t->roots_cap) {
    uint64_t cap = std::max<uint64_t>(t->roots_cap, 1024);
    while (cap < want) cap *= 2;
    cap += 1;   // sizes 0 .. cap-1: a full tree of 2^k leaves has 2^k + 1 of them
    Fr* nw = nullptr;
    HIP_TRY(hipMalloc((void**)&nw, cap * sizeof(Fr)));
    if (t->d_roots) {
      hipError_t e = t->roots_done ? hipMemcpyAsync(nw, t->d_roots, t->roots_done * sizeof(Fr), hipMemcpyDeviceToDevice, st) : hipSuccess;
      if (e == hipSuccess) e = hipStreamSynchronize(st);
      if (e != hipSuccess) {
        hipFree(nw);
        return fail(SPP_ERR_HIP, "prefix roots: %s", hipGetErrorString(e));
      }
      hipFree(t->d_roots);
    }
    t->d_roots = nw;
    t->roots_cap = cap;
  }
  while (t->roots_done < want) {
    const uint32_t chunk = (uint32_t)std::min<uint64_t>(want - t->roots_done, (uint64_t)1 << 30);
    launch_prefix_roots(st, ctx->hc, t->dev, t->roots_done, chunk, t->d_roots + t->roots_done);
    t->roots_done += chunk;
  }
  return SPP_OK;
}
extern "C" int spp_merkle_tree_prefix_roots(spp_merkle_tree* t, uint64_t first_size, size_t count, uint8_t* roots) {
  if (!t || (count && !roots)) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count > (1u << 24)) return fail(SPP_ERR_BAD_INPUT, "too many sizes in one call (%zu; at most 2^24)", count);
  spp_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  if (count == 0 ? first_size > t->n_leaves : (first_size > t->n_leaves || count - 1 > t->n_leaves - first_size))
    return fail(SPP_ERR_BAD_INPUT, "sizes %llu .. %llu reach past the tree, which has %llu leaves", (unsigned long long)first_size,
                (unsigned long long)(first_size + count - (count ? 1 : 0)), (unsigned long long)t->n_leaves);
  if (count == 0) return SPP_OK;
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  hipStream_t st = ctx->stream;
  if (int e = mt_roots_sync(t)) return e;
  DevBuf dout;
  HIP_TRY(dout.alloc(count * 32));
  launch_fr_to_be(st, t->d_roots + first_size, dout.as<uint8_t>(), (uint32_t)count);
  HIP_TRY(hipMemcpyAsync(roots, dout.p, count * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}
// The root index over R (leaf_index.hpp: same table, same fence, the tree's salt), brought up to the tree, then one query launch.
// A word >= r is the encoding of no field element: it is answered here, and a zero word is queried in its place.  ctx->mu held,
// device set, constants ready.
static int mt_find_roots(spp_merkle_tree* t, size_t count, const uint8_t* roots, uint64_t* sizes, uint32_t* matches) {
  if (t->n_leaves > LEAF_INDEX_MAX_LEAVES)
    return fail(SPP_ERR_BAD_INPUT, "the tree has %llu leaves: the root index covers at most 2^30", (unsigned long long)t->n_leaves);
  hipStream_t st = t->ctx->stream;
  if (int e = mt_roots_sync(t)) return e;
  const uint64_t entries = t->n_leaves + 1;
  // 2^30 + 1 entries in 2^31 slots: a little over half full, which the probing does not mind (it needs one empty slot)
  const uint32_t want = entries > LEAF_INDEX_MAX_LEAVES ? 1u << 31 : leaf_index_slots(entries);
  LeafIndex ix;
  if (int e = mt_table_sync(t, &t->d_root_index, &t->root_index_slots, &t->roots_indexed, t->d_roots, entries, want, &ix)) return e;
  std::vector<uint8_t> keys(roots, roots + 32 * count);
  std::vector<size_t> foreign;
  for (size_t i = 0; i < count; i++)
    if (!be_is_canonical<FrParams>(roots + 32 * i)) {
      foreign.push_back(i);
      memset(keys.data() + 32 * i, 0, 32);
    }
  DevBuf dk, di, dm;
  UP(dk, keys.data(), count * 32);
  HIP_TRY(di.alloc(count * sizeof(uint64_t)));
  if (matches) HIP_TRY(dm.alloc(count * sizeof(uint32_t)));
  launch_leaf_find(st, ix, t->d_roots, dk.as<uint8_t>(), nullptr, di.as<uint64_t>(), matches ? dm.as<uint32_t>() : nullptr, (uint32_t)count);
  HIP_TRY(hipMemcpyAsync(sizes, di.p, count * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
  if (matches) HIP_TRY(hipMemcpyAsync(matches, dm.p, count * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  for (size_t i : foreign) {
    sizes[i] = SPP_TREE_NO_SIZE;
    if (matches) matches[i] = 0;
  }
  return SPP_OK;
}
extern "C" int spp_merkle_tree_find_roots(spp_merkle_tree* t, size_t count, const uint8_t* roots, uint64_t* sizes, uint32_t* matches) {
  if (!t || (count && (!roots || !sizes))) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count == 0) return SPP_OK;
  if (count > (1u << 24)) return fail(SPP_ERR_BAD_INPUT, "too many roots in one call (%zu; at most 2^24)", count);
  spp_ctx* ctx = t->ctx;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  return mt_find_roots(t, count, roots, sizes, matches);
}
extern "C" int spp_pool_root_sizes(spp_pool* pool, spp_merkle_tree* t, uint64_t sizes[33], uint64_t* best) {
  if (!pool || !t || !sizes) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  spp_ctx* ctx = t->ctx;
  if (spp_pool_view(pool, nullptr, nullptr) != ctx) return fail(SPP_ERR_BAD_INPUT, "the pool belongs to another spp_ctx than the tree");
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  uint8_t words[33 * 32];
  spp_pool_ring_words(pool, words);
  uint64_t found[33];
  if (int e = mt_find_roots(t, 33, words, found, nullptr)) return e;
  uint64_t top = SPP_TREE_NO_SIZE;
  for (int k = 0; k < 33; k++) {
    sizes[k] = found[k];
    if (found[k] != SPP_TREE_NO_SIZE && (top == SPP_TREE_NO_SIZE || found[k] > top)) top = found[k];
  }
  if (best) *best = top;
  return SPP_OK;
}

extern "C" int spp_grumpkin_keygen_batch(spp_ctx* ctx, size_t count, const uint8_t* sk, uint8_t* xy) {
  if (!ctx || !sk || !xy) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count == 0) return SPP_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  hipStream_t st = ctx->stream;
  DevBuf ds, dx;
  UP(ds, sk, count * 32);
  HIP_TRY(dx.alloc(count * 64));
  launch_grumpkin_keygen(st, ctx->gk_table, ds.as<uint8_t>(), dx.as<uint8_t>(), (uint32_t)count);
  HIP_TRY(hipMemcpyAsync(xy, dx.p, count * 64, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}

extern "C" int spp_poseidon2_sponge_batch(spp_ctx* ctx, size_t count, uint32_t n, const uint8_t* in, uint8_t* out) {
  if (!ctx || !in || !out) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count == 0) return SPP_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  hipStream_t st = ctx->stream;
  DevBuf di, dout;
  UP(di, in, count * n * 32);
  HIP_TRY(dout.alloc(count * 32));
  launch_poseidon2_sponge(st, ctx->hc, di.as<uint8_t>(), n, dout.as<uint8_t>(), (uint32_t)count);
  HIP_TRY(hipMemcpyAsync(out, dout.p, count * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}
// -----------------------------------------------------------------------------------------------------
// audit inputs end to end on the device: (sk, r, e1, e2) -> 3360-field rows for spp_prove_batch(_device)
// -----------------------------------------------------------------------------------------------------
namespace {
struct ScratchPiece {
  void* p = nullptr;
  template <class T> T* as() { return (T*)p; }
};
const size_t AUDIT_PIECES = 10;
void audit_piece_sizes(size_t count, size_t sizes[AUDIT_PIECES]) {
  const size_t v[AUDIT_PIECES] = {count * 64, count * 64, count * 64 * 4, count * 1024 * 4, count * 64 * 4, count * 1024 * 4, count * 157 * 32, count * 32,
                                  count * 32, sizeof(RlwePkDev)};
  for (size_t i = 0; i < AUDIT_PIECES; i++) sizes[i] = (v[i] + 255) / 256 * 256;
}
}  // namespace
size_t spp_audit_scratch_bytes(size_t count) {
  size_t sizes[AUDIT_PIECES], total = 0;
  audit_piece_sizes(count, sizes);
  for (size_t sz : sizes) total += sz;
  return total;
}
// Enqueues the whole input pipeline of scripts/generate_audit.py:468-641 on `st` (no synchronisation): the rows are complete
// for whatever is enqueued on `st` next.  scratch: spp_audit_scratch_bytes(count) bytes of device memory that stay untouched
// until those kernels have run.  d_c0_out / d_c1_out (optional, count * 64 / count * 1024 u32): the ciphertext c0 / c1 of every
// instance (generate_audit.py:590-606), written by the RLWE kernel itself.
int spp_audit_inputs_enqueue(spp_ctx* ctx, hipStream_t st, void* scratch, const uint32_t* d_pk_a, const uint32_t* d_pk_b, uint32_t count,
                             const uint8_t* d_sk, const int8_t* d_r, const int8_t* d_e1, const int8_t* d_e2, uint8_t* d_rows, uint32_t* d_c0_out,
                             uint32_t* d_c1_out) {
  ScratchPiece xy, msg, c0, c1, k0, k1, packed, ct, wa, pkhat;
  {
    size_t sizes[AUDIT_PIECES], off = 0;
    audit_piece_sizes(count, sizes);
    ScratchPiece* pieces[AUDIT_PIECES] = {&xy, &msg, &c0, &c1, &k0, &k1, &packed, &ct, &wa, &pkhat};
    for (size_t i = 0; i < AUDIT_PIECES; i++) {
      pieces[i]->p = (uint8_t*)scratch + off;
      off += sizes[i];
    }
  }
  if (int e = spp_ensure_rlwe(ctx)) return e;
  RlweDev rd = ctx->rlwe;
  rd.pk = pkhat.as<RlwePkDev>();   // the transformed public key of THIS call (calls in flight on other streams may use other keys)
  // the ciphertext is read by nothing after the RLWE kernel (the rows take the packed form): a caller that wants it gets it
  // written in place of the scratch pieces, at no extra traffic
  if (d_c0_out) c0.p = d_c0_out;
  if (d_c1_out) c1.p = d_c1_out;
  launch_grumpkin_keygen(st, ctx->gk_table, d_sk, xy.as<uint8_t>(), count);                       // generate_audit.py:482
  launch_poseidon_hash(st, ctx->hc, xy.as<uint8_t>(), 2, wa.as<uint8_t>(), count);                 // wa_commitment
  launch_audit_msg(st, xy.as<uint8_t>(), msg.as<uint8_t>(), count);                                // :489-496
  launch_rlwe_witness(st, rd, d_pk_a, d_pk_b, d_r, d_e1, d_e2, msg.as<uint8_t>(), c0.as<uint32_t>(), c1.as<uint32_t>(), k0.as<int32_t>(),
                      k1.as<int32_t>(), packed.as<uint8_t>(), count);                              // :507-584
  launch_poseidon2_sponge(st, ctx->hc, packed.as<uint8_t>(), 157, ct.as<uint8_t>(), count);        // ct_commitment :587
  launch_audit_assemble(st, wa.as<uint8_t>(), ct.as<uint8_t>(), packed.as<uint8_t>(), d_sk, d_r, d_e1, d_e2, k0.as<int32_t>(),
                        k1.as<int32_t>(), d_rows, count);                                          // Prover.toml order :630-641
  return SPP_OK;
}
static int audit_inputs_on_device(spp_ctx* ctx, const uint32_t* d_pk_a, const uint32_t* d_pk_b, uint32_t count, const uint8_t* d_sk,
                                  const int8_t* d_r, const int8_t* d_e1, const int8_t* d_e2, uint8_t* d_rows) {
  hipStream_t st = ctx->stream;
  // temporaries kept between calls (grow only): a hipFree per call would drain every stream of the device
  const size_t total = spp_audit_scratch_bytes(count);
  if (total > ctx->audit_scratch_cap) {
    if (ctx->audit_scratch) HIP_TRY(hipFree(ctx->audit_scratch));
    ctx->audit_scratch = nullptr;
    ctx->audit_scratch_cap = 0;
    HIP_TRY(hipMalloc(&ctx->audit_scratch, total));
    ctx->audit_scratch_cap = total;
  }
  if (int e = spp_audit_inputs_enqueue(ctx, st, ctx->audit_scratch, d_pk_a, d_pk_b, count, d_sk, d_r, d_e1, d_e2, d_rows, nullptr, nullptr)) return e;
  HIP_TRY(hipStreamSynchronize(st));   // the rows are complete when the call returns (the caller hands them to a proving stream)
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}
extern "C" int spp_audit_inputs_batch_device(spp_ctx* ctx, const void* d_pk_a, const void* d_pk_b, size_t count, const void* d_sk,
                                             const void* d_r, const void* d_e1, const void* d_e2, void* d_rows) {
  if (!ctx || !d_pk_a || !d_pk_b || !d_sk || !d_r || !d_e1 || !d_e2 || !d_rows) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count == 0) return SPP_OK;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  return audit_inputs_on_device(ctx, (const uint32_t*)d_pk_a, (const uint32_t*)d_pk_b, (uint32_t)count, (const uint8_t*)d_sk,
                                (const int8_t*)d_r, (const int8_t*)d_e1, (const int8_t*)d_e2, (uint8_t*)d_rows);
}
extern "C" int spp_audit_inputs_batch(spp_ctx* ctx, const uint32_t* pk_a, const uint32_t* pk_b, size_t count, const uint8_t* sk,
                                      const int8_t* r, const int8_t* e1, const int8_t* e2, uint8_t* rows) {
  if (!ctx || !pk_a || !pk_b || !sk || !r || !e1 || !e2 || !rows) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count == 0) return SPP_OK;
  for (int i = 0; i < 1024; i++)
    if (pk_a[i] >= 167772161u || pk_b[i] >= 167772161u) return fail(SPP_ERR_BAD_INPUT, "public key coefficient not in [0, q)");
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  if (int e = spp_ensure_ctx_consts(ctx)) return e;
  hipStream_t st = ctx->stream;
  DevBuf da, db, ds, dr, de1, de2, drows;
  UP(da, pk_a, 4096); UP(db, pk_b, 4096); UP(ds, sk, count * 32);
  UP(dr, r, count * 1024); UP(de1, e1, count * 64); UP(de2, e2, count * 1024);
  HIP_TRY(drows.alloc(count * 3360 * 32));
  if (int e = audit_inputs_on_device(ctx, da.as<uint32_t>(), db.as<uint32_t>(), (uint32_t)count, ds.as<uint8_t>(), dr.as<int8_t>(),
                                     de1.as<int8_t>(), de2.as<int8_t>(), drows.as<uint8_t>()))
    return e;
  HIP_TRY(hipMemcpy(rows, drows.p, count * 3360 * 32, hipMemcpyDeviceToHost));
  return SPP_OK;
}

// -----------------------------------------------------------------------------------------------------
// auditor side: Shamir reconstruction of the RLWE secret key, batch decryption of audit ciphertexts
// -----------------------------------------------------------------------------------------------------
extern "C" int spp_shamir_reconstruct(spp_ctx* ctx, uint32_t t, const uint32_t* xs, const uint8_t* ys, size_t n, uint8_t* secret_be,
                                      uint32_t* sk_mod_q) {
  if (!ctx || !xs || !ys || (!secret_be && !sk_mod_q)) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (t == 0 || t > 64) return fail(SPP_ERR_BAD_INPUT, "threshold out of range");
  for (uint32_t i = 0; i < t; i++)
    for (uint32_t j = 0; j < i; j++)
      if (xs[i] == xs[j]) return fail(SPP_ERR_BAD_INPUT, "duplicate share index");
  if (n == 0) return SPP_OK;
  // Lagrange coefficients at 0: lambda_i = prod_{j != i} (-x_j) / (x_i - x_j)   (rlwe_decrypt.py:38-51)
  std::vector<Fr> lam(t);
  for (uint32_t i = 0; i < t; i++) {
    Fr num = Fr::one(), den = Fr::one();
    for (uint32_t j = 0; j < t; j++) {
      if (i == j) continue;
      num = num * Fr::from_u64(xs[j]).neg();
      den = den * (Fr::from_u64(xs[i]) - Fr::from_u64(xs[j]));
    }
    lam[i] = num * den.inv();
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf dl, dy, ds, dq;
  UP(dl, lam.data(), sizeof(Fr) * t);
  UP(dy, ys, (size_t)t * n * 32);
  if (secret_be) HIP_TRY(ds.alloc(n * 32));
  if (sk_mod_q) HIP_TRY(dq.alloc(n * 4));
  launch_shamir_combine(st, dl.as<Fr>(), dy.as<uint8_t>(), t, (uint32_t)n, secret_be ? ds.as<uint8_t>() : nullptr,
                        sk_mod_q ? dq.as<uint32_t>() : nullptr);
  if (secret_be) HIP_TRY(hipMemcpyAsync(secret_be, ds.p, n * 32, hipMemcpyDeviceToHost, st));
  if (sk_mod_q) HIP_TRY(hipMemcpyAsync(sk_mod_q, dq.p, n * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}

extern "C" int spp_rlwe_decrypt_batch(spp_ctx* ctx, const uint32_t* sk_mod_q, size_t count, const uint32_t* c0, const uint32_t* c1,
                                      uint8_t* msg) {
  if (!ctx || !sk_mod_q || !c0 || !c1 || !msg) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count == 0) return SPP_OK;
  for (int i = 0; i < 1024; i++)
    if (sk_mod_q[i] >= 167772161u) return fail(SPP_ERR_BAD_INPUT, "secret key coefficient not in [0, q)");
  // k_rlwe_decrypt takes the coefficients as they are: its 64-bit sums are sized for values below q (audit_open.hpp).  A record
  // that may be malformed is opened by spp_audit_open_batch, which reduces the coefficient and flags the record.
  for (size_t k = 0; k < count; k++) {
    for (int i = 0; i < 64; i++)
      if (c0[k * 64 + i] >= 167772161u) return fail(SPP_ERR_BAD_INPUT, "ciphertext %zu: c0[%d] not in [0, q)", k, i);
    for (int i = 0; i < 1024; i++)
      if (c1[k * 1024 + i] >= 167772161u) return fail(SPP_ERR_BAD_INPUT, "ciphertext %zu: c1[%d] not in [0, q)", k, i);
  }
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  DevBuf dsk, d0, d1, dm;
  UP(dsk, sk_mod_q, 4096); UP(d0, c0, count * 64 * 4); UP(d1, c1, count * 1024 * 4);
  HIP_TRY(dm.alloc(count * 64));
  launch_rlwe_decrypt(st, dsk.as<uint32_t>(), d0.as<uint32_t>(), d1.as<uint32_t>(), dm.as<uint8_t>(), (uint32_t)count);
  HIP_TRY(hipMemcpyAsync(msg, dm.p, count * 64, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}

// -----------------------------------------------------------------------------------------------------
// auditor key generation (scripts/rlwe_keygen.py:98-182): sampling on the host, the key pair and its check on the device, the
// Shamir sharing of the secret key (:51-65).  Everything that held the secret key or the sharing polynomials is wiped.
// -----------------------------------------------------------------------------------------------------
namespace {
const uint32_t RLWE_Q = 167772161u;
const size_t KEYGEN_MAX_KEYS = (size_t)1 << 16, SHAMIR_MAX_VALUES = (size_t)1 << 20;
int check_below_q(const char* what, const uint32_t* v, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (v[i] >= RLWE_Q) return fail(SPP_ERR_BAD_INPUT, "%s[%zu] = %u is not in [0, q)", what, i, v[i]);
  return SPP_OK;
}
}  // namespace

extern "C" int spp_rlwe_sample_key(size_t count, uint32_t bound, int8_t* sk, uint32_t* a, int8_t* e) {
  if (!sk || !a || !e) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (bound < 1 || bound > 127) return fail(SPP_ERR_BAD_INPUT, "bound %u is not in [1, 127]", bound);
  if (count > KEYGEN_MAX_KEYS) return fail(SPP_ERR_BAD_INPUT, "count %zu: at most 2^16 keys in one call", count);
  OsRandom rnd;
  const uint32_t range = 2 * bound + 1, limit = 256 - 256 % range;   // bytes below `limit` are uniform mod range
  const size_t n = count * 1024;
  for (int8_t* dst : {sk, e})
    for (size_t i = 0; i < n;) {
      uint8_t v;
      if (!rnd.next(&v, 1)) return fail(SPP_ERR_IO, "cannot read /dev/urandom");
      if (v < limit) dst[i++] = (int8_t)((int)(v % range) - (int)bound);
    }
  for (size_t i = 0; i < n;) {
    uint8_t w[4];
    if (!rnd.next(w, 4)) return fail(SPP_ERR_IO, "cannot read /dev/urandom");
    const uint32_t v = ((uint32_t)w[0] | (uint32_t)w[1] << 8 | (uint32_t)w[2] << 16 | (uint32_t)w[3] << 24) & 0x0fffffffu;   // q < 2^28
    if (v < RLWE_Q) a[i++] = v;
  }
  return SPP_OK;
}

extern "C" int spp_rlwe_keygen_batch(spp_ctx* ctx, size_t count, const int8_t* sk, const uint32_t* a, const int8_t* e, uint32_t* pk_b,
                                     uint32_t* sk_mod_q) {
  if (!ctx || !sk || !a || !e || !pk_b) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count > KEYGEN_MAX_KEYS) return fail(SPP_ERR_BAD_INPUT, "count %zu: at most 2^16 keys in one call", count);
  if (count == 0) return SPP_OK;
  if (int rc = check_below_q("a", a, count * 1024)) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (int rc = spp_ensure_rlwe(ctx)) return rc;
  const size_t n = count * 1024;
  WipedDevBuf dsk, dskq;
  DevBuf da, de, db;
  UP_SECRET(dsk, sk, n);
  UP(da, a, n * 4); UP(de, e, n);
  HIP_TRY(db.alloc(n * 4));
  if (sk_mod_q) {
    dskq.bytes = n * 4; dskq.st = st;
    HIP_TRY(dskq.alloc(n * 4));
  }
  launch_rlwe_keygen(st, ctx->rlwe, dsk.as<int8_t>(), da.as<uint32_t>(), de.as<int8_t>(), db.as<uint32_t>(),
                     sk_mod_q ? dskq.as<uint32_t>() : nullptr, (uint32_t)count);
  HIP_TRY(hipMemcpyAsync(pk_b, db.p, n * 4, hipMemcpyDeviceToHost, st));
  if (sk_mod_q) HIP_TRY(hipMemcpyAsync(sk_mod_q, dskq.p, n * 4, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}

extern "C" int spp_rlwe_key_check(spp_ctx* ctx, size_t count, const uint32_t* pk_a, const uint32_t* pk_b, const uint32_t* sk_mod_q,
                                  uint32_t* max_abs) {
  if (!ctx || !pk_a || !pk_b || !sk_mod_q || !max_abs) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (count > KEYGEN_MAX_KEYS) return fail(SPP_ERR_BAD_INPUT, "count %zu: at most 2^16 keys in one call", count);
  if (count == 0) return SPP_OK;
  const size_t n = count * 1024;
  if (int rc = check_below_q("pk_a", pk_a, n)) return rc;
  if (int rc = check_below_q("pk_b", pk_b, n)) return rc;
  if (int rc = check_below_q("sk_mod_q", sk_mod_q, n)) return rc;
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  if (int rc = spp_ensure_rlwe(ctx)) return rc;
  WipedDevBuf dsk;
  DevBuf da, db, dm;
  UP_SECRET(dsk, sk_mod_q, n * 4);
  UP(da, pk_a, n * 4); UP(db, pk_b, n * 4);
  HIP_TRY(dm.alloc(count * 8));
  launch_rlwe_key_noise(st, ctx->rlwe, da.as<uint32_t>(), db.as<uint32_t>(), dsk.as<uint32_t>(), dm.as<uint32_t>(), (uint32_t)count);
  HIP_TRY(hipMemcpyAsync(max_abs, dm.p, count * 8, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}

extern "C" int spp_shamir_split(spp_ctx* ctx, uint32_t t, uint32_t m, const uint32_t* xs, size_t n, const uint8_t* secrets_be,
                                const uint8_t* coeffs_be, uint8_t* ys) {
  if (!ctx || !secrets_be || !ys) return fail(SPP_ERR_BAD_INPUT, "NULL argument");
  if (t == 0 || t > 64) return fail(SPP_ERR_BAD_INPUT, "threshold %u is not in [1, 64]", t);
  if (m < t || m > 255) return fail(SPP_ERR_BAD_INPUT, "%u shares: need between the threshold %u and 255", m, t);
  if (xs)
    for (uint32_t j = 0; j < m; j++) {
      if (xs[j] == 0) return fail(SPP_ERR_BAD_INPUT, "xs[%u] is 0: that share would be the secret", j);
      for (uint32_t k = 0; k < j; k++)
        if (xs[k] == xs[j]) return fail(SPP_ERR_BAD_INPUT, "xs[%u] repeats xs[%u] = %u", j, k, xs[j]);
    }
  if (n > SHAMIR_MAX_VALUES) return fail(SPP_ERR_BAD_INPUT, "n %zu: at most 2^20 values in one call", n);
  if (n == 0) return SPP_OK;
  for (size_t i = 0; i < n; i++)
    if (!be_is_canonical<FrParams>(secrets_be + 32 * i)) return fail(SPP_ERR_BAD_INPUT, "secret %zu is not a canonical field element", i);
  const size_t ncoef = (size_t)(t - 1) * n;
  if (coeffs_be)
    for (size_t i = 0; i < ncoef; i++)
      if (!be_is_canonical<FrParams>(coeffs_be + 32 * i))
        return fail(SPP_ERR_BAD_INPUT, "coefficient %zu (x^%zu of value %zu) is not a canonical field element", i, i / n + 1, i % n);
  // the sharing polynomials from the OS when the caller brings none
  WipedBytes drawn;
  if (!coeffs_be && ncoef) {
    drawn.v.resize(ncoef * 32);
    OsRandom rnd;
    if (int rc = draw_field_elements(rnd, drawn.v.data(), ncoef)) return rc;
    coeffs_be = drawn.v.data();
  }
  std::vector<Fr> x(m);
  for (uint32_t j = 0; j < m; j++) x[j] = Fr::from_u64(xs ? xs[j] : j + 1);
  std::lock_guard<std::mutex> lk(ctx->mu);
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  WipedDevBuf ds, dc;
  DevBuf dx, dy;
  UP(dx, x.data(), sizeof(Fr) * m);
  UP_SECRET(ds, secrets_be, n * 32);
  UP_SECRET(dc, coeffs_be, ncoef * 32);
  HIP_TRY(dy.alloc((size_t)m * n * 32));
  launch_shamir_split(st, dx.as<Fr>(), ds.as<uint8_t>(), dc.as<uint8_t>(), t, m, (uint32_t)n, dy.as<uint8_t>());
  HIP_TRY(hipMemcpyAsync(ys, dy.p, (size_t)m * n * 32, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  return SPP_OK;
}
