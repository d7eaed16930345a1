/* N-API binding of libspp's C ABI (include/spp.h) for the TypeScript host code.
 * Replaces the two execSync() calls of the reference's client/proof.helper.ts:55,64 with in-process calls.
 * Synchronous, like the reference; errors become thrown JS Errors whose message carries the SPP_ERR_* code. */
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "../../include/spp.h"

#define NAPI_OK(call)                                            \
  do {                                                           \
    if ((call) != napi_ok) {                                     \
      napi_throw_error(env, NULL, "N-API call failed: " #call);  \
      return NULL;                                               \
    }                                                            \
  } while (0)

static napi_value throw_spp(napi_env env, int code) {
  char msg[640];
  snprintf(msg, sizeof msg, "libspp error %d: %s", code, spp_last_error());
  napi_throw_error(env, NULL, msg);
  return NULL;
}
static char* get_string(napi_env env, napi_value v) {
  size_t len = 0;
  if (napi_get_value_string_utf8(env, v, NULL, 0, &len) != napi_ok) return NULL;
  char* s = (char*)malloc(len + 1);
  napi_get_value_string_utf8(env, v, s, len + 1, &len);
  return s;
}

static spp_ctx* g_ctx = NULL;

/* init(device) */
static napi_value Init(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  int32_t dev = 0;
  if (argc >= 1) napi_get_value_int32(env, argv[0], &dev);
  if (!g_ctx) {
    int rc = spp_init(dev, &g_ctx);
    if (rc) return throw_spp(env, rc);
  }
  napi_value r;
  napi_get_boolean(env, 1, &r);
  return r;
}
/* buildCircuit(id, outPath, auxUint32Array?) -> nbConstraints */
static napi_value BuildCircuit(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  int32_t id = 0;
  napi_get_value_int32(env, argv[0], &id);
  char* path = get_string(env, argv[1]);
  const uint32_t* aux = NULL;
  if (argc >= 3) {
    bool is_ta = false;
    napi_is_typedarray(env, argv[2], &is_ta);
    if (is_ta) {
      napi_typedarray_type t;
      size_t len;
      void* data;
      napi_get_typedarray_info(env, argv[2], &t, &len, &data, NULL, NULL);
      if (t == napi_uint32_array && len == 2048) aux = (const uint32_t*)data;
    }
  }
  uint32_t n = 0;
  int rc = spp_circuit_build(id, aux, path, &n);
  free(path);
  if (rc) return throw_spp(env, rc);
  napi_value r;
  napi_create_uint32(env, n, &r);
  return r;
}
/* setup(circuitPath, seed32 Buffer, pkPath, vkPath) */
static napi_value Setup(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (!g_ctx) { napi_throw_error(env, NULL, "call init() first"); return NULL; }
  char* c = get_string(env, argv[0]);
  void* seed; size_t slen;
  NAPI_OK(napi_get_buffer_info(env, argv[1], &seed, &slen));
  char* pk = get_string(env, argv[2]);
  char* vk = get_string(env, argv[3]);
  int rc = slen == 32 ? spp_setup(g_ctx, c, (const uint8_t*)seed, pk, vk) : SPP_ERR_BAD_INPUT;
  free(c); free(pk); free(vk);
  if (rc) return throw_spp(env, rc);
  return NULL;
}
static void finalize_circuit(napi_env env, void* data, void* hint) { (void)env; (void)hint; spp_free_circuit((spp_circuit*)data); }
/* loadCircuit(circuitPath, pkPath, windowBits) -> handle */
static napi_value LoadCircuit(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (!g_ctx) { napi_throw_error(env, NULL, "call init() first"); return NULL; }
  char* c = get_string(env, argv[0]);
  char* pk = get_string(env, argv[1]);
  int32_t wb = 0;
  if (argc >= 3) napi_get_value_int32(env, argv[2], &wb);
  spp_circuit* h = NULL;
  int rc = spp_load_circuit(g_ctx, c, pk, wb, &h);
  free(c); free(pk);
  if (rc) return throw_spp(env, rc);
  napi_value ext;
  NAPI_OK(napi_create_external(env, h, finalize_circuit, NULL, &ext));
  return ext;
}
/* circuitInfo(handle) -> Uint32 array of 8 */
static napi_value CircuitInfo(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  void* h;
  NAPI_OK(napi_get_value_external(env, argv[0], &h));
  uint32_t inf[8];
  int rc = spp_circuit_info((spp_circuit*)h, inf);
  if (rc) return throw_spp(env, rc);
  napi_value arr;
  napi_create_array_with_length(env, 8, &arr);
  for (uint32_t i = 0; i < 8; i++) { napi_value v; napi_create_uint32(env, inf[i], &v); napi_set_element(env, arr, i, v); }
  return arr;
}
/* proveBatch(handle, count, inputs Buffer, rs Buffer|null) -> {proofs, publicWitnesses, status} */
static napi_value ProveBatch(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  void* h;
  NAPI_OK(napi_get_value_external(env, argv[0], &h));
  uint32_t count = 0;
  napi_get_value_uint32(env, argv[1], &count);
  void* in; size_t inlen;
  NAPI_OK(napi_get_buffer_info(env, argv[2], &in, &inlen));
  void* rs = NULL; size_t rslen = 0;
  bool isbuf = false;
  if (argc >= 4) napi_is_buffer(env, argv[3], &isbuf);
  if (isbuf) NAPI_OK(napi_get_buffer_info(env, argv[3], &rs, &rslen));
  uint32_t inf[8];
  spp_circuit_info((spp_circuit*)h, inf);
  size_t pwlen = 12 + 32 * (size_t)inf[1];
  if (inlen != (size_t)count * inf[6] * 32 || (rs && rslen != (size_t)count * 64)) {
    napi_throw_error(env, NULL, "libspp error -1: input buffer has the wrong length");
    return NULL;
  }
  void *proofs, *pws;
  napi_value bproofs, bpws, st, out;
  NAPI_OK(napi_create_buffer(env, (size_t)count * SPP_PROOF_LEN, &proofs, &bproofs));
  NAPI_OK(napi_create_buffer(env, (size_t)count * pwlen, &pws, &bpws));
  int32_t* status = (int32_t*)calloc(count ? count : 1, sizeof(int32_t));
  int rc = spp_prove_batch((spp_circuit*)h, count, (const uint8_t*)in, (const uint8_t*)rs, (uint8_t*)proofs, (uint8_t*)pws, status);
  if (rc && rc != SPP_ERR_UNSAT) { free(status); return throw_spp(env, rc); }
  napi_create_array_with_length(env, count, &st);
  for (uint32_t i = 0; i < count; i++) { napi_value v; napi_create_int32(env, status[i], &v); napi_set_element(env, st, i, v); }
  free(status);
  napi_create_object(env, &out);
  napi_set_named_property(env, out, "proofs", bproofs);
  napi_set_named_property(env, out, "publicWitnesses", bpws);
  napi_set_named_property(env, out, "status", st);
  return out;
}
/* verify(vk Buffer, proof Buffer, publicWitness Buffer) -> boolean   (`sunspot verify`, prove_linux.sh:86-87; host only) */
static napi_value Verify(napi_env env, napi_callback_info info) {
  size_t argc = 3;
  napi_value argv[3];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  void *vk, *pr, *pw;
  size_t vkl, prl, pwl;
  NAPI_OK(napi_get_buffer_info(env, argv[0], &vk, &vkl));
  NAPI_OK(napi_get_buffer_info(env, argv[1], &pr, &prl));
  NAPI_OK(napi_get_buffer_info(env, argv[2], &pw, &pwl));
  int ok = 0;
  int rc = spp_verify((const uint8_t*)vk, vkl, (const uint8_t*)pr, prl, (const uint8_t*)pw, pwl, &ok);
  if (rc) return throw_spp(env, rc);
  napi_value r;
  napi_get_boolean(env, ok != 0, &r);
  return r;
}
/* verifyBatch(vk Buffer, count, proofs Buffer, publicWitnesses Buffer) -> boolean[]   (after init(); one GPU lane per proof) */
static napi_value VerifyBatch(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (!g_ctx) { napi_throw_error(env, NULL, "call init() first"); return NULL; }
  void* ctx = g_ctx;
  void *vk, *pr, *pw;
  size_t vkl, prl, pwl;
  NAPI_OK(napi_get_buffer_info(env, argv[0], &vk, &vkl));
  uint32_t count = 0;
  napi_get_value_uint32(env, argv[1], &count);
  NAPI_OK(napi_get_buffer_info(env, argv[2], &pr, &prl));
  NAPI_OK(napi_get_buffer_info(env, argv[3], &pw, &pwl));
  if (prl != (size_t)count * SPP_PROOF_LEN || (count && pwl % count)) {
    napi_throw_error(env, NULL, "libspp error -1: proof / public-witness buffer has the wrong length");
    return NULL;
  }
  int32_t* ok = (int32_t*)calloc(count ? count : 1, sizeof(int32_t));
  int rc = spp_verify_batch((spp_ctx*)ctx, (const uint8_t*)vk, vkl, count, (const uint8_t*)pr, (const uint8_t*)pw, count ? pwl / count : 12, ok,
                            NULL);
  if (rc) { free(ok); return throw_spp(env, rc); }
  napi_value arr;
  napi_create_array_with_length(env, count, &arr);
  for (uint32_t i = 0; i < count; i++) { napi_value v; napi_get_boolean(env, ok[i] != 0, &v); napi_set_element(env, arr, i, v); }
  free(ok);
  return arr;
}
/* ---- the pool's Merkle tree resident in HBM (spp_merkle_tree_*), in the context init() made (the one loadCircuit uses) ----
 * The handle is an external over a tagged box, so that a circuit handle passed as a tree is refused rather than misread. */
#define TREE_MAGIC 0x74726565u
typedef struct {
  uint32_t magic, depth;
  spp_merkle_tree* t;
} tree_box;
static void finalize_tree(napi_env env, void* data, void* hint) {
  (void)env; (void)hint;
  tree_box* b = (tree_box*)data;
  spp_merkle_tree_free(b->t);
  free(b);
}
static tree_box* get_tree(napi_env env, napi_value v) {
  void* p = NULL;
  napi_valuetype type;
  if (napi_typeof(env, v, &type) != napi_ok || type != napi_external || napi_get_value_external(env, v, &p) != napi_ok || !p ||
      ((tree_box*)p)->magic != TREE_MAGIC) {
    napi_throw_error(env, NULL, "libspp error -1: not a tree handle (treeNew)");
    return NULL;
  }
  return (tree_box*)p;
}
static napi_value make_uint64(napi_env env, uint64_t v) {   /* sizes and indices stay below 2^53 (depth <= 32) */
  napi_value r;
  napi_create_double(env, (double)v, &r);
  return r;
}
/* treeNew(depth) -> tree handle */
static napi_value TreeNew(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  if (!g_ctx) { napi_throw_error(env, NULL, "call init() first"); return NULL; }
  uint32_t depth = SPP_TREE_DEPTH;
  if (argc >= 1) napi_get_value_uint32(env, argv[0], &depth);
  spp_merkle_tree* t = NULL;
  int rc = spp_merkle_tree_new(g_ctx, depth, &t);
  if (rc) return throw_spp(env, rc);
  tree_box* b = (tree_box*)malloc(sizeof *b);
  b->magic = TREE_MAGIC;
  b->depth = depth;
  b->t = t;
  napi_value ext;
  if (napi_create_external(env, b, finalize_tree, NULL, &ext) != napi_ok) {
    finalize_tree(env, b, NULL);
    napi_throw_error(env, NULL, "N-API call failed: napi_create_external");
    return NULL;
  }
  return ext;
}
/* treeSize(tree) -> number of leaves */
static napi_value TreeSize(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  tree_box* b = get_tree(env, argv[0]);
  if (!b) return NULL;
  return make_uint64(env, spp_merkle_tree_size(b->t));
}
/* treeInsert(tree, leaves Buffer of n * 32 B) -> index of the first leaf */
static napi_value TreeInsert(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  tree_box* b = get_tree(env, argv[0]);
  if (!b) return NULL;
  void* in; size_t len;
  NAPI_OK(napi_get_buffer_info(env, argv[1], &in, &len));
  if (len % 32) { napi_throw_error(env, NULL, "libspp error -1: leaves must be 32 bytes each"); return NULL; }
  uint64_t first = 0;
  int rc = spp_merkle_tree_insert(b->t, len / 32, (const uint8_t*)in, &first);
  if (rc) return throw_spp(env, rc);
  return make_uint64(env, first);
}
/* treeRoot(tree) -> Buffer(32) */
static napi_value TreeRoot(napi_env env, napi_callback_info info) {
  size_t argc = 1;
  napi_value argv[1];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  tree_box* b = get_tree(env, argv[0]);
  if (!b) return NULL;
  void* out;
  napi_value buf;
  NAPI_OK(napi_create_buffer(env, 32, &out, &buf));
  int rc = spp_merkle_tree_root(b->t, (uint8_t*)out);
  if (rc) return throw_spp(env, rc);
  return buf;
}
/* treeProofs(tree, indices number[]) -> Buffer(n * depth * 32): the siblings of every index, leaf level first */
static napi_value TreeProofs(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  tree_box* b = get_tree(env, argv[0]);
  if (!b) return NULL;
  uint32_t n = 0;
  NAPI_OK(napi_get_array_length(env, argv[1], &n));
  uint64_t* idx = (uint64_t*)calloc(n ? n : 1, sizeof(uint64_t));
  for (uint32_t i = 0; i < n; i++) {
    napi_value v;
    double d = -1;
    napi_get_element(env, argv[1], i, &v);
    napi_get_value_double(env, v, &d);
    if (!(d >= 0 && d < 18446744073709551616.0) || d != (double)(uint64_t)d) {
      free(idx);
      napi_throw_error(env, NULL, "libspp error -1: an index is not a non-negative integer");
      return NULL;
    }
    idx[i] = (uint64_t)d;
  }
  void* out;
  napi_value buf;
  size_t depth_bytes = (size_t)32 * b->depth;
  if (napi_create_buffer(env, (size_t)n * depth_bytes, &out, &buf) != napi_ok) {
    free(idx);
    napi_throw_error(env, NULL, "N-API call failed: napi_create_buffer");
    return NULL;
  }
  int rc = spp_merkle_tree_proofs(b->t, n, idx, (uint8_t*)out);
  free(idx);
  if (rc) return throw_spp(env, rc);
  return buf;
}
/* treeDeposit(tree, deposits Buffer of n * SPP_DEPOSIT_LEN B) -> {first, commitments Buffer(n * 32), roots Buffer(n * 32)} */
static napi_value TreeDeposit(napi_env env, napi_callback_info info) {
  size_t argc = 2;
  napi_value argv[2];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  tree_box* b = get_tree(env, argv[0]);
  if (!b) return NULL;
  void* in; size_t len;
  NAPI_OK(napi_get_buffer_info(env, argv[1], &in, &len));
  if (len % SPP_DEPOSIT_LEN) { napi_throw_error(env, NULL, "libspp error -1: deposits must be 96 bytes each"); return NULL; }
  const size_t n = len / SPP_DEPOSIT_LEN;
  void *com, *roots;
  napi_value bcom, broots, out;
  NAPI_OK(napi_create_buffer(env, n * 32, &com, &bcom));
  NAPI_OK(napi_create_buffer(env, n * 32, &roots, &broots));
  uint64_t first = 0;
  int rc = spp_merkle_tree_deposit(b->t, n, (const uint8_t*)in, &first, (uint8_t*)com, (uint8_t*)roots);
  if (rc) return throw_spp(env, rc);
  napi_create_object(env, &out);
  napi_set_named_property(env, out, "first", make_uint64(env, first));
  napi_set_named_property(env, out, "commitments", bcom);
  napi_set_named_property(env, out, "roots", broots);
  return out;
}
/* proveWithdrawNotes(circuit, tree, notes Buffer of n * SPP_NOTE_LEN B, rs Buffer|null) -> {proofs, publicWitnesses, status}
 * (spp_prove_withdraw_notes: every proof against the tree's root at the time of the call) */
static napi_value ProveWithdrawNotes(napi_env env, napi_callback_info info) {
  size_t argc = 4;
  napi_value argv[4];
  NAPI_OK(napi_get_cb_info(env, info, &argc, argv, NULL, NULL));
  void* h;
  NAPI_OK(napi_get_value_external(env, argv[0], &h));
  tree_box* b = get_tree(env, argv[1]);
  if (!b) return NULL;
  void* notes; size_t nlen;
  NAPI_OK(napi_get_buffer_info(env, argv[2], &notes, &nlen));
  void* rs = NULL; size_t rslen = 0;
  bool isbuf = false;
  if (argc >= 4) napi_is_buffer(env, argv[3], &isbuf);
  if (isbuf) NAPI_OK(napi_get_buffer_info(env, argv[3], &rs, &rslen));
  const size_t count = nlen / SPP_NOTE_LEN;
  if (nlen % SPP_NOTE_LEN || (rs && rslen != count * 64)) {
    napi_throw_error(env, NULL, "libspp error -1: notes / rs buffer has the wrong length");
    return NULL;
  }
  uint32_t inf[8];
  int rc = spp_circuit_info((spp_circuit*)h, inf);
  if (rc) return throw_spp(env, rc);
  size_t pwlen = 12 + 32 * (size_t)inf[1];
  void *proofs, *pws;
  napi_value bproofs, bpws, st, out;
  NAPI_OK(napi_create_buffer(env, count * SPP_PROOF_LEN, &proofs, &bproofs));
  NAPI_OK(napi_create_buffer(env, count * pwlen, &pws, &bpws));
  int32_t* status = (int32_t*)calloc(count ? count : 1, sizeof(int32_t));
  rc = spp_prove_withdraw_notes((spp_circuit*)h, b->t, count, (const uint8_t*)notes, (const uint8_t*)rs, (uint8_t*)proofs, (uint8_t*)pws, status);
  if (rc && rc != SPP_ERR_UNSAT) { free(status); return throw_spp(env, rc); }
  napi_create_array_with_length(env, count, &st);
  for (size_t i = 0; i < count; i++) { napi_value v; napi_create_int32(env, status[i], &v); napi_set_element(env, st, (uint32_t)i, v); }
  free(status);
  napi_create_object(env, &out);
  napi_set_named_property(env, out, "proofs", bproofs);
  napi_set_named_property(env, out, "publicWitnesses", bpws);
  napi_set_named_property(env, out, "status", st);
  return out;
}
static napi_value Version(napi_env env, napi_callback_info info) {
  (void)info;
  napi_value r;
  napi_create_string_utf8(env, spp_version(), NAPI_AUTO_LENGTH, &r);
  return r;
}

static napi_value ModuleInit(napi_env env, napi_value exports) {
  napi_property_descriptor d[] = {
      {"init", NULL, Init, NULL, NULL, NULL, napi_default, NULL},
      {"buildCircuit", NULL, BuildCircuit, NULL, NULL, NULL, napi_default, NULL},
      {"setup", NULL, Setup, NULL, NULL, NULL, napi_default, NULL},
      {"loadCircuit", NULL, LoadCircuit, NULL, NULL, NULL, napi_default, NULL},
      {"circuitInfo", NULL, CircuitInfo, NULL, NULL, NULL, napi_default, NULL},
      {"proveBatch", NULL, ProveBatch, NULL, NULL, NULL, napi_default, NULL},
      {"verify", NULL, Verify, NULL, NULL, NULL, napi_default, NULL},
      {"verifyBatch", NULL, VerifyBatch, NULL, NULL, NULL, napi_default, NULL},
      {"version", NULL, Version, NULL, NULL, NULL, napi_default, NULL},
      {"treeNew", NULL, TreeNew, NULL, NULL, NULL, napi_default, NULL},
      {"treeSize", NULL, TreeSize, NULL, NULL, NULL, napi_default, NULL},
      {"treeInsert", NULL, TreeInsert, NULL, NULL, NULL, napi_default, NULL},
      {"treeRoot", NULL, TreeRoot, NULL, NULL, NULL, napi_default, NULL},
      {"treeProofs", NULL, TreeProofs, NULL, NULL, NULL, napi_default, NULL},
      {"treeDeposit", NULL, TreeDeposit, NULL, NULL, NULL, napi_default, NULL},
      {"proveWithdrawNotes", NULL, ProveWithdrawNotes, NULL, NULL, NULL, napi_default, NULL},
  };
  napi_define_properties(env, exports, sizeof d / sizeof d[0], d);
  return exports;
}
NAPI_MODULE(spp_addon, ModuleInit)
