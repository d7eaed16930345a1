// Host build of csrc/pool_table.hpp (g++, no GPU): the ring, the slot function and probing of a resident set, and the resolve
// rule, driven from stdin by tests/test_pool_host.py, which compares every line with its own sequential model.
//   ring <n> <q>          then n roots and q queries (hex, one per line)      -> state bytes (hex), then q chars 0/1
//   table <salt> <cap> <n> <q>   then n keys to import and q queries          -> "slots <count>", per key "<home> <slot|dup>", q chars 0/1
//   resolve <salt> <dup> <n>     then n lines "<key> <prov> <valid>"          -> n final codes, space separated
//                                prov: p = pending on its proof, r = fails with BAD_RECIPIENT unless displaced, 0..6 = already final
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pool_table.hpp"

using namespace spp;

static bool unhex(const char* s, uint8_t* out, size_t n) {
  if (strlen(s) != 2 * n) return false;
  for (size_t i = 0; i < n; i++) {
    unsigned v;
    if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
    out[i] = (uint8_t)v;
  }
  return true;
}
static bool read_key(uint8_t* out) {
  char buf[128];
  return scanf("%100s", buf) == 1 && unhex(buf, out, 32);
}

int main() {
  char cmd[32];
  while (scanf("%31s", cmd) == 1) {
    if (!strcmp(cmd, "ring")) {
      unsigned n, q;
      if (scanf("%u %u", &n, &q) != 2) return 2;
      PoolState st;
      pool_state_init(st);
      uint8_t key[32];
      for (unsigned i = 0; i < n; i++) {
        if (!read_key(key)) return 2;
        pool_add_root(st, key);
      }
      uint8_t bytes[POOL_STATE_LEN];
      pool_state_bytes(st, bytes);
      for (unsigned i = 0; i < POOL_STATE_LEN; i++) printf("%02x", bytes[i]);
      printf("\n");
      for (unsigned i = 0; i < q; i++) {
        if (!read_key(key)) return 2;
        putchar(pool_check_root(st, key) ? '1' : '0');
      }
      printf("\n");
    } else if (!strcmp(cmd, "table")) {
      unsigned long long salt, cap;
      unsigned n, q;
      if (scanf("%llx %llu %u %u", &salt, &cap, &n, &q) != 4) return 2;
      const uint32_t slots = pool_slots_for(cap);
      std::vector<uint32_t> claim(slots, 0);
      std::vector<uint8_t> keys((size_t)slots * 32, 0);
      PoolSet set{claim.data(), keys.data(), slots - 1};
      printf("slots %u\n", slots);
      uint8_t key[32];
      for (unsigned i = 0; i < n; i++) {
        if (!read_key(key)) return 2;
        const uint32_t home = pool_slot(key, salt, set.mask);
        if (pool_set_contains(set, salt, key))
          printf("%u dup\n", home);
        else
          printf("%u %u\n", home, pool_set_insert_unique(set, salt, key));
      }
      for (unsigned i = 0; i < q; i++) {
        if (!read_key(key)) return 2;
        putchar(pool_set_contains(set, salt, key) ? '1' : '0');
      }
      printf("\n");
    } else if (!strcmp(cmd, "resolve")) {
      unsigned long long salt;
      int dup;
      unsigned n;
      if (scanf("%llx %d %u", &salt, &dup, &n) != 3) return 2;
      const size_t stride = 40;   // keys sit inside a wider record, as they do in a public witness
      std::vector<uint8_t> buf(stride * n + 8, 0xEE);
      std::vector<int32_t> prov(n);
      std::vector<int> valid(n);
      for (unsigned i = 0; i < n; i++) {
        char pc[8];
        if (!read_key(buf.data() + 8 + stride * i) || scanf("%7s %d", pc, &valid[i]) != 2) return 2;
        prov[i] = pc[0] == 'p' ? POOL_PENDING_PROOF : pc[0] == 'r' ? pool_pending_refused(POOL_BAD_RECIPIENT) : atoi(pc);
      }
      const uint8_t* keys = buf.data() + 8;
      const uint32_t rs = pool_slots_for(n);
      std::vector<uint32_t> slots(rs, POOL_NONE);
      // the claims in an order of their own (descending): the result must not depend on it
      for (unsigned k = n; k-- > 0;)
        if (pool_is_candidate(prov[k], valid[k] != 0)) pool_resolve_claim(slots.data(), rs - 1, salt, keys, stride, k);
      for (unsigned i = 0; i < n; i++) {
        const uint32_t w = prov[i] >= 0 ? POOL_NONE : pool_resolve_winner(slots.data(), rs - 1, salt, keys, stride, i);
        printf("%d%c", pool_final_code(prov[i], valid[i] != 0, w, i, dup), i + 1 == n ? '\n' : ' ');
      }
    } else {
      return 2;
    }
  }
  return 0;
}
