// Host build of the log pieces of csrc/pool_table.hpp (g++, no GPU): the ring at a position and the whole rule of a log in which
// deposits, submit_audits and withdraws alternate, in the order spp_pool_settle_log launches them (audit screen, claim, settle;
// withdraw screen at each position; claim, settle; both commits), driven from stdin by tests/test_pool_log_host.py, which compares
// every line with the sequential model.
//   ringat <T0> <n> <q>     then T0 resident roots, n batch roots, q queries (hex, one per line)
//                           -> the state bytes after all T0 + n pushes (hex), then for d = 0..n a line of q chars 0/1: check_root
//                              after the resident pushes and the first d batch roots
//   log <salt> <cap> <pre> <n>   then pre lines "R <root>" | "A <wa key>" | "N <nullifier>" (the state at the call) and n lines
//                           "d <root>" | "a <pw, 76 B> <valid>" | "w <pw, 172 B> <address> <valid>"
//                           -> n final codes; n amounts; the state bytes; the nullifier set's keys; the audit set's keys ("-": none)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pool_table.hpp"

using namespace spp;

static bool read_hex(uint8_t* out, size_t n) {
  static char buf[1024];
  if (scanf("%1000s", buf) != 1 || strlen(buf) != 2 * n) return false;
  for (size_t i = 0; i < n; i++) {
    unsigned v;
    if (sscanf(buf + 2 * i, "%2x", &v) != 1) return false;
    out[i] = (uint8_t)v;
  }
  return true;
}
static void print_hex(const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; i++) printf("%02x", p[i]);
}
static void print_state(const PoolState& st) {
  uint8_t bytes[POOL_STATE_LEN];
  pool_state_bytes(st, bytes);
  print_hex(bytes, POOL_STATE_LEN);
  printf("\n");
}
// (ring entries of st) | roots: what spp_pool_settle_log uploads for the withdraws
static std::vector<uint8_t> ring_of(const PoolState& st, const std::vector<uint8_t>& roots) {
  std::vector<uint8_t> ring(POOL_ROOTS * 32 + roots.size());
  pool_ring_entries(st, ring.data());
  if (!roots.empty()) memcpy(ring.data() + POOL_ROOTS * 32, roots.data(), roots.size());
  return ring;
}

struct HostSet {
  std::vector<uint32_t> claim;
  std::vector<uint8_t> keys;
  PoolSet set;
  explicit HostSet(uint64_t cap) : claim(pool_slots_for(cap), 0), keys((size_t)pool_slots_for(cap) * 32, 0) {
    set = PoolSet{claim.data(), keys.data(), pool_slots_for(cap) - 1};
  }
  void print() const {
    bool any = false;
    for (size_t s = 0; s < claim.size(); s++)
      if (claim[s]) {
        if (any) printf(" ");
        print_hex(keys.data() + s * 32, 32);
        any = true;
      }
    fputs(any ? "\n" : "-\n", stdout);
  }
};

// claims in descending order (an order of their own: the result must not depend on it), then every final code
static void resolve(uint64_t salt, const uint8_t* keys, size_t stride, const std::vector<int32_t>& prov, const std::vector<int>& valid, int32_t dup,
                    std::vector<uint32_t>& slots, std::vector<int32_t>& result) {
  const uint32_t n = (uint32_t)prov.size();
  slots.assign(pool_slots_for(n), POOL_NONE);
  const uint32_t mask = (uint32_t)slots.size() - 1;
  for (uint32_t k = n; k-- > 0;)
    if (pool_is_candidate(prov[k], valid[k] != 0)) pool_resolve_claim(slots.data(), mask, salt, keys, stride, k);
  result.resize(n);
  for (uint32_t i = 0; i < n; i++) {
    const uint32_t w = prov[i] >= 0 ? POOL_NONE : pool_resolve_winner(slots.data(), mask, salt, keys, stride, i);
    result[i] = pool_final_code(prov[i], valid[i] != 0, w, i, dup);
  }
}

int main() {
  char cmd[32];
  while (scanf("%31s", cmd) == 1) {
    if (!strcmp(cmd, "ringat")) {
      unsigned t0, n, q;
      if (scanf("%u %u %u", &t0, &n, &q) != 3) return 2;
      PoolState st;
      pool_state_init(st);
      uint8_t key[32];
      for (unsigned i = 0; i < t0; i++) {
        if (!read_hex(key, 32)) return 2;
        pool_add_root(st, key);
      }
      std::vector<uint8_t> roots((size_t)n * 32), queries((size_t)q * 32);
      for (unsigned i = 0; i < n; i++)
        if (!read_hex(roots.data() + 32 * i, 32)) return 2;
      for (unsigned i = 0; i < q; i++)
        if (!read_hex(queries.data() + 32 * i, 32)) return 2;
      const std::vector<uint8_t> ring = ring_of(st, roots);   // from the state at the call, as the library takes it
      for (unsigned i = 0; i < n; i++) pool_add_root(st, roots.data() + 32 * i);
      print_state(st);
      for (unsigned d = 0; d <= n; d++) {
        for (unsigned i = 0; i < q; i++) putchar(pool_check_root_at(ring.data(), d, queries.data() + 32 * i) ? '1' : '0');
        printf("\n");
      }
    } else if (!strcmp(cmd, "log")) {
      unsigned long long salt, cap;
      unsigned pre, n;
      if (scanf("%llx %llu %u %u", &salt, &cap, &pre, &n) != 4) return 2;
      PoolState st;
      pool_state_init(st);
      HostSet nullifiers(cap), audits(cap);
      uint8_t key[32];
      for (unsigned i = 0; i < pre; i++) {
        char k[4];
        if (scanf("%3s", k) != 1 || !read_hex(key, 32)) return 2;
        if (k[0] == 'R')
          pool_add_root(st, key);
        else if (!pool_set_contains(k[0] == 'A' ? audits.set : nullifiers.set, salt, key))
          pool_set_insert_unique(k[0] == 'A' ? audits.set : nullifiers.set, salt, key);
      }
      std::vector<uint8_t> kinds(n), roots, apws, wpws, addresses;
      std::vector<int> avalid, wvalid;
      for (unsigned i = 0; i < n; i++) {
        char k[4];
        int v;
        if (scanf("%3s", k) != 1) return 2;
        if (k[0] == 'd') {
          kinds[i] = POOL_INSTR_DEPOSIT;
          roots.resize(roots.size() + 32);
          if (!read_hex(roots.data() + roots.size() - 32, 32)) return 2;
        } else if (k[0] == 'a') {
          kinds[i] = POOL_INSTR_SUBMIT_AUDIT;
          apws.resize(apws.size() + POOL_AUDIT_PW);
          if (!read_hex(apws.data() + apws.size() - POOL_AUDIT_PW, POOL_AUDIT_PW) || scanf("%d", &v) != 1) return 2;
          avalid.push_back(v);
        } else if (k[0] == 'w') {
          kinds[i] = POOL_INSTR_WITHDRAW;
          wpws.resize(wpws.size() + POOL_WITHDRAW_PW);
          addresses.resize(addresses.size() + 32);
          if (!read_hex(wpws.data() + wpws.size() - POOL_WITHDRAW_PW, POOL_WITHDRAW_PW) || !read_hex(addresses.data() + addresses.size() - 32, 32) ||
              scanf("%d", &v) != 1)
            return 2;
          wvalid.push_back(v);
        } else {
          return 2;
        }
      }
      size_t cnt[3];
      if (!pool_log_index(kinds.data(), n, cnt, 0, 0, nullptr, nullptr, nullptr, nullptr)) return 2;
      if (cnt[0] * 32 != roots.size() || cnt[1] != avalid.size() || cnt[2] != wvalid.size()) return 3;
      const uint32_t na = (uint32_t)cnt[1], nw = (uint32_t)cnt[2];
      std::vector<uint32_t> apos(na), wpos(nw), wdep(nw), waud(nw);
      pool_log_index(kinds.data(), n, cnt, na, nw, apos.data(), wpos.data(), wdep.data(), waud.data());
      const std::vector<uint8_t> ring = ring_of(st, roots);
      const uint8_t* akeys = apws.data() + POOL_A_WA;
      const uint8_t* wkeys = wpws.data() + POOL_W_NULLIFIER;
      // the submit_audits among themselves
      std::vector<int32_t> aprov(na), wprov(nw), aresult, wresult;
      std::vector<uint32_t> aslots, wslots;
      for (uint32_t r = 0; r < na; r++) aprov[r] = pool_screen_audit(audits.set, salt, apws.data() + (size_t)r * POOL_AUDIT_PW);
      resolve(salt, akeys, POOL_AUDIT_PW, aprov, avalid, POOL_AUDIT_EXISTS, aslots, aresult);
      // the withdraws, each at its position; the audit set is still the one of the call
      const PoolLogView view{ring.data(), aslots.data(), (uint32_t)aslots.size() - 1, akeys, POOL_AUDIT_PW};
      std::vector<unsigned long long> amounts(n, 0);
      for (uint32_t r = 0; r < nw; r++) {
        const uint8_t* pw = wpws.data() + (size_t)r * POOL_WITHDRAW_PW;
        amounts[wpos[r]] = pool_amount_u64(pw);
        wprov[r] = pool_screen_withdraw_at(view, wdep[r], waud[r], audits.set, nullifiers.set, salt, pw, addresses.data() + (size_t)r * 32);
      }
      resolve(salt, wkeys, POOL_WITHDRAW_PW, wprov, wvalid, POOL_NULLIFIER_USED, wslots, wresult);
      // the commits, then log order
      std::vector<int32_t> result(n, POOL_OK);
      for (uint32_t r = 0; r < na; r++) {
        if (aresult[r] == POOL_OK) pool_set_insert_unique(audits.set, salt, akeys + (size_t)r * POOL_AUDIT_PW);
        result[apos[r]] = aresult[r];
      }
      for (uint32_t r = 0; r < nw; r++) {
        if (wresult[r] == POOL_OK) pool_set_insert_unique(nullifiers.set, salt, wkeys + (size_t)r * POOL_WITHDRAW_PW);
        result[wpos[r]] = wresult[r];
      }
      for (size_t i = 0; i < cnt[0]; i++) pool_add_root(st, roots.data() + 32 * i);
      for (unsigned i = 0; i < n; i++) printf("%d%c", result[i], i + 1 == n ? '\n' : ' ');
      for (unsigned i = 0; i < n; i++) printf("%llu%c", amounts[i], i + 1 == n ? '\n' : ' ');
      if (n == 0) printf("\n\n");
      print_state(st);
      nullifiers.print();
      audits.print();
    } else {
      return 2;
    }
  }
  return 0;
}
