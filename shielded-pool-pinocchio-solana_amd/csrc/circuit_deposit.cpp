// Deposit circuit -- R1CS for "this commitment, hiding this amount, was appended at this index to the tree of this root".
//
// The reference has no such circuit: its program reads the commitment of a deposit and ignores it, pushes whatever new_root the
// client sent and transfers an amount nothing ties to the commitment (shielded_pool_program/src/instructions/deposit.rs:31-36,73).
// This statement is what a program -- or an indexer, relayer or auditor reading a deposit log -- would check instead.
//
//   public : old_root, new_root, commitment, amount, index      (.pw order; five words, as the withdraw circuit)
//   private: owner_x, owner_y, randomness, siblings[depth]
//
//   1. amount is a u64 (eight byte limbs, looked up)                                     main.nr:43
//   2. commitment == Poseidon(owner_x, owner_y, amount, randomness)                      main.nr:69-70, client/merkle.ts:126-133
//   3. bits = the `depth` bits of index, so index < 2^depth
//   4. two Merkle chains over the same bits and the same siblings (main.nr:11-29), written as build_withdraw_circuit writes its
//      one: from the constant 0, the empty leaf (client/merkle.ts:152), to old_root; from commitment to new_root.
//
// No secret key and no Grumpkin ladder: a payroll employer deposits to an owner whose key it does not hold.  An owner that is not
// a point of the curve makes a note no withdraw proof can spend (main.nr:54-62 derives the owner from the key): the depositor's
// loss, nobody else's.
//
// index is public on purpose.  The verifier keeps a leaf counter and requires index == counter and old_root == its current root;
// then "the leaf at index was empty under old_root and is commitment under new_root, every sibling unchanged" is the whole
// statement of an append, and nothing has to be said about the siblings to the right.  Without the counter a depositor could fill
// any empty slot and every client tree (insert = push, merkle.ts:159-163) would part from the chain's root.
//
// The constant leaf.  The first hash of the empty chain takes  left = 0 + bit * (sibling - 0),  right = sibling - that product:
// the selection wire comes before the hash, so neither operand of the permutation is a constant, the hint rows read ordinary
// linear forms and no S-box has a constant on its B side.  Nothing had to be pinned to a wire.
#include "circuit.hpp"

namespace spp {

Circuit build_deposit_circuit(bool native_hints, uint32_t depth) {
  Builder b(CIRCUIT_DEPOSIT);
  LC old_root = b.public_input();
  LC new_root = b.public_input();
  LC commitment = b.public_input();
  LC amount = b.public_input();
  LC index = b.public_input();
  LC owner_x = b.secret_input();
  LC owner_y = b.secret_input();
  LC randomness = b.secret_input();
  std::vector<LC> siblings;
  for (uint32_t i = 0; i < depth; i++) siblings.push_back(b.secret_input());

  // 1. amount: pub u64
  b.to_limbs8(amount, 8);

  // 2. the commitment opens to (owner, amount, randomness)
  b.assert_eq(gadget_poseidon_hash(b, {owner_x, owner_y, amount, randomness}, native_hints), commitment);

  // 3. + 4. the slot was empty under old_root and holds the commitment under new_root
  std::vector<LC> path = b.to_bits(index, depth);
  LC cur[2] = {LC(), commitment};
  for (uint32_t i = 0; i < depth; i++)
    for (int k = 0; k < 2; k++) {
      LC d = b.mul(path[i], siblings[i] - cur[k]);  // bit ? sibling-cur : 0
      LC left = cur[k] + d;
      LC right = siblings[i] - d;
      cur[k] = gadget_poseidon_hash(b, {left, right}, native_hints);
    }
  b.assert_eq(cur[0], old_root);
  b.assert_eq(cur[1], new_root);
  return b.finish();
}

}  // namespace spp
