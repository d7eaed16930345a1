"""`spp` command line: the four sunspot sub-commands the reference's scripts call, same positional arguments and
output-file naming (outputs land next to the circuit file, as sunspot writes them next to the .ccs).

    python -m spp.cli compile withdraw|audit [--rlwe-pk rlwe_pk.json] -o target/<name>.sppc     # prints nbConstraints=<n>
    python -m spp.cli compile target/<name>.json [-o target/<name>.sppc]                          # sunspot compile <acir>: the
                                                                                                  # nargo-compiled program itself
    python -m spp.cli setup   target/<name>.sppc [--seed HEX32] [--force]                         # -> <name>.pk, <name>.vk (+ .setup.json;
                                                                                                  #    skipped when the keys match the circuit)
    python -m spp.cli prove   target/<name>.sppc target/<name>.pk Prover.toml                    # -> <name>.proof, <name>.pw
    python -m spp.cli verify  target/<name>.vk target/<name>.proof target/<name>.pw              # exit 0 / 1
    python -m spp.cli verify-batch target/<name>.vk <a>.proof <a>.pw [<b>.proof <b>.pw ...]      # `sunspot verify` in a loop, on the GPU
                              # by random linear combination (spp_verify_batch_rlc, seed from the OS): one verdict per pair,
                              # exit 0 iff all verify
    python -m spp.cli audit-open target/<name>.vk|- <name>.proof <name>.pw ciphertext.json --shares share_1.json share_2.json
                              # the auditor's `python scripts/rlwe_decrypt.py`: reconstructs the key from the shares, verifies the
                              # proof (`-`: already verified elsewhere), checks that the ciphertext is the one the proof commits
                              # to and that it decrypts to the identity the proof commits to; exit 0 only if all three hold
    python -m spp.cli audit-open target/<name>.vk|- <name>.proof <name>.pw ciphertext.json --partials partial_1.json partial_2.json
                              # the same from the auditors' partial decryptions: nobody rebuilds the key (exactly one of --shares
                              # and --partials); a fourth line reports whether the partials belong together
    python -m spp.cli audit-pair-seeds --shares M --out DIR
                              # DIR/pair_seeds_<i>.json for the auditors 1..M: one 32-byte seed from the operating system per pair,
                              # the same value at both ends; file i goes to auditor i alone, over the channel its share took
    python -m spp.cli audit-partial share_i.json --with X1 X2 ... ciphertext.json <name>.pw [--pair-seeds pair_seeds_i.json]
                              [--smudge B] --out partial_i.json
                              # auditor i's partial decryption of one record within the set {i, X1, X2, ...}, from its own share:
                              # masked with the pair seeds, smudged with noise in [-B, B] (default 1024; threshold * B <= 2^17).
                              # Refuses a ciphertext that is not the one the public witness commits to
    python -m spp.cli rlwe-keygen --out DIR [--threshold 2 --shares 3] [--reference-seed N]
                              # `python scripts/rlwe_keygen.py`: DIR/rlwe_pk.json, DIR/rlwe_params.json and
                              # DIR/rlwe_sk_shares/share_<i>.json, from the operating system's randomness; then checks its own
                              # files on the GPU (reconstructs the key from the first `threshold` shares, both noise maxima)
    python -m spp.cli rlwe-key-check rlwe_pk.json --shares share_1.json share_2.json [--params rlwe_params.json]
                              # are these shares the secret of this public key?  prints max |b + a*sk| and max |sk| (centred),
                              # exit 0 iff both are within the noise bound of rlwe_params.json (next to rlwe_pk.json; default 3)
    python -m spp.cli dkg-deal --index I --threshold T --shares M --a-seed HEX32 --out DIR [--refresh]
                              # auditor I's part of a key that no dealer ever holds: draws its own s_I, e_I from the operating system,
                              # computes b_I = e_I - a*s_I (a from the seed the auditors agreed on) and deals s_I to the auditors 1..M
                              # with public commitments.  Writes DIR/deal_<I>.json (public), DIR/deal_<I>.hash (its SHA-256: every
                              # auditor publishes this BEFORE any deal file is revealed) and DIR/private/subshare_<I>_to_<J>.json
                              # (for auditor J alone).  --refresh: a dealing of zero that renews the shares of an existing key.
                              # M <= 10: the noise of M summed keys, M * 18432 + 3, and the smudging limit 2^17 stay below delta / 2
    python -m spp.cli dkg-receive --index J --deals deal_1.json ... --hashes deal_1.hash ... --subshares subshare_1_to_J.json ...
                              --out DIR [--refresh share_J.json]
                              # auditor J checks every dealer's file against the hash published first (--hashes in the order of
                              # --deals) and every sub-share against the commitments, on the GPU; then writes DIR/rlwe_pk.json,
                              # DIR/rlwe_params.json and DIR/rlwe_sk_shares/share_<J>.json, the files of rlwe-keygen (--refresh: only
                              # the share, the old one plus the dealt zeros).  exit 1 names the first failing dealer, the check
                              # (hash, missing, agreement, point, share, not-zero) and the value; nothing is written then
    python -m spp.cli dkg-committee --deals deal_1.json ... [--base committee.json] --out committee.json
                              # the committee's commitments, the sums of the dealers' (no secrets): key dealings make the file,
                              # refresh dealings are added to --base.  Checks what dkg-receive checks of the public files; exit 1
                              # names the dealer and the value of a commitment that is no point
    python -m spp.cli dkg-reshare-deal --share share_J.json (--blind blind_J.json | --subshares F...) --committee committee.json
                              --set X1 .. Xt --new-threshold T --new-shares M --out DIR
                              # old member J of the set deals its share to a new committee of M at threshold T (M <= 255: the key and
                              # its noise stay, so dkg-deal's limit of 10 does not apply).  First checks (share, blind) against the
                              # committee file on the GPU: exit 1 `share-mismatch`, nothing written.  Writes DIR/reshare_<J>.json
                              # (public) and DIR/private/subshare_<J>_to_<K>.json
    python -m spp.cli dkg-reshare-receive --index K --committee committee.json --deals reshare_*.json --subshares ... --out DIR
                              # new member K checks every sub-share against its dealer's commitments and every dealer's constant
                              # terms against the old committee file, on the GPU; then writes DIR/rlwe_sk_shares/share_<K>.json,
                              # DIR/private/blind_<K>.json, DIR/committee.json and DIR/rlwe_params.json (rlwe_pk.json stays).  exit 1
                              # names the first failing old member, the check (set, missing, agreement, point, share, not-share)
                              # and the value; nothing is written then
    python -m spp.cli pool-replay withdraw.vk audit.vk log.jsonl [--capacity N] [--verifier each|rlc [--group N]]
                              # the pool program's decisions for a log of instructions, one JSON object per line, values in hex:
                              #   {"deposit": {"root"}}  {"submit_audit": {"proof", "pw"}}  {"withdraw": {"proof", "pw", "recipient"}}
                              # prints one result name per line (OK, AUDIT_EXISTS, NO_AUDIT_RECORD, BAD_ROOT, NULLIFIER_USED,
                              # BAD_RECIPIENT, BAD_PROOF; a deposit only pushes its root and prints OK).  --verifier rlc checks
                              # the proofs by random linear combination (spp_pool_set_verifier): the same lines.
                              # A deposit may carry "commitment" beside "root" (all deposits of a log or none; --depth of the tree,
                              # default 16): the leaves then go into a resident tree and a deposit's line reads `OK root-of-leaves`
                              # or `OK NOT-root-of-leaves` (the program takes new_root as sent, instructions/deposit.rs:31-36,73),
                              # an accepted withdraw's `OK size <n>` -- the size of the leaf list whose root it used -- or
                              # `OK foreign`, and a closing `roots:` line counts both
    python -m spp.cli wallet-sync secrets.json leaves.txt [--spent nullifiers.txt] [--audited wa.txt] [--vk withdraw.vk audit.vk] [--recipient HEX]
                              # a wallet's DepositRecords (demo-frontend/app/lib/storage.ts:9-26) from its secrets -- a JSON list of
                              # {"secretKey", "amount", "randomness"} -- and the chain's leaves, one hex leaf per line in chain order
                              # (MerkleTreeState.leaves, :45-50).  --spent / --audited: the nullifier and wa_commitment accounts the
                              # pool holds, one hex key per line (they go through spp_pool_import_keys and need --vk).  Prints one
                              # JSON object per secret: commitment, leafIndex, root, nullifier, waCommitment, siblings, publicKeyX/Y,
                              # status ("pending" | "withdrawn"; "absent" with leafIndex null when the commitment is no leaf), audited
                              # (null without --vk) and occurrences -- the form importDeposits (:233-260) reads
    python -m spp.cli withdraw-bundle notes.jsonl withdraw.sppc withdraw.pk audit.sppc audit.pk rlwe_pk.json leaves.txt --out DIR
                              [--audited wa.txt --vk withdraw.vk audit.vk] [--size N] [--with-deposits]
                              # everything the relayer posts for the notes `wallet-sync --recipient` printed (demo-frontend/app/api/
                              # relay/withdraw/route.ts:129-287): the withdraw proof of every note and ONE audit record per identity
                              # that has none yet -- none for the wa_commitments of --audited (spp_prove_withdrawals).  Writes
                              # DIR/log.jsonl in the relayer's order (a note's submit_audit, if it is the one that carries its
                              # identity's record, then its withdraw), which pool-replay takes, and per record DIR/record_<s>.proof,
                              # record_<s>.pw and ciphertext_<s>.json, which audit-open takes.  --with-deposits: the log begins with
                              # the deposits of all leaves.  exit 1 if the circuit refused a row
    python -m spp.cli compile deposit -o deposit.sppc                                           # the deposit circuit (include/spp.h)
    python -m spp.cli deposit-prove deposits.jsonl deposit.sppc deposit.pk leaves.txt --out DIR
                              # deposits.jsonl: one {"secretKey", "amount", "randomness"} per line; leaves.txt: the chain's leaves so
                              # far, one hex leaf per line (may be empty).  Appends the deposits to a resident depth-16 tree and proves
                              # each one (old_root, new_root, commitment, amount, index public).  Writes DIR/deposit_<i>.proof / .pw,
                              # i = the leaf index, and DIR/log.jsonl with one line per deposit
                              #   {"deposit": {"root", "commitment", "amount", "proof", "pw"}}
                              # which deposit-verify takes and pool-replay reads as a deposit with a commitment (it ignores the other
                              # keys).  The reference's program does not verify these proofs.  exit 1 if the circuit refused a row
    python -m spp.cli deposit-verify deposit.vk log.jsonl [--start-root HEX --start-index N]
                              # the log checked as a program keeping (current_root, leaf count) would, from the empty tree or the
                              # given state: per line the pw amount against "amount", old_root against the current root, index
                              # against the count, the proof; an accepted line advances the state, a rejected one does not.  Prints
                              # one result name per line (OK, BAD_AMOUNT, STALE_ROOT, BAD_INDEX, BAD_PROOF); exit 1 names the first
                              # line that is not OK
    python -m spp.cli setup-contribute <name>.pk <name>.vk --out DIR [--entropy HEX32]
                              # one contribution to a setup ceremony: multiplies the key's delta by a secret drawn from the operating
                              # system (--entropy: for reproducible tests only) and writes DIR/<name>.pk, DIR/<name>.vk and
                              # DIR/<name>.receipt; prints the SHA-256 of the receipt, which the contributor publishes
    python -m spp.cli setup-verify <pk0> <vk0> <pk1> <vk1> <receipt1> [<pk2> <vk2> <receipt2> ...]
                              # a chain of contributions, link by link: exit 0 if every link is a contribution to the key before it,
                              # else exit 1 naming the first failing link and its reason (FORMAT, NOT_A_DELTA_CHANGE, POINT_INVALID,
                              # RECEIPT, DELTA_PAIR, SCALING, VK)
    python -m spp.cli ptau-new <log> --out <name>.ptau
                              # the first phase of a ceremony starts here: the powers-of-tau transcript of tau = alpha = beta = 1 for
                              # domains up to 2^log (host only)
    python -m spp.cli ptau-contribute <name>.ptau --out DIR [--entropy HEX32]
                              # one contribution to the transcript: multiplies tau, alpha and beta by secrets drawn from the operating
                              # system (--entropy: for reproducible tests only) and writes DIR/<name>.ptau and DIR/<name>.receipt;
                              # prints the SHA-256 of the receipt, which the contributor publishes
    python -m spp.cli ptau-verify <t0> <t1> <receipt1> [<t2> <receipt2> ...]
                              # a chain of transcript contributions, link by link: exit 0 if every link is a contribution to the
                              # transcript before it, else exit 1 naming the first failing link and its reason (FORMAT, SIZE,
                              # POINT_INVALID, RECEIPT, TAU_G1, TAU_G2, ALPHA, BETA)
    python -m spp.cli setup-derive <name>.sppc <name>.ptau --out DIR
                              # the circuit's keys from a transcript of at least its domain size, no secret involved: DIR/<name>.pk
                              # and DIR/<name>.vk with gamma = delta = sigma = 1; checking a published derivation is re-running it
    python -m spp.cli setup-contribute-sigma <name>.pk <name>.vk --out DIR [--entropy HEX32]
    python -m spp.cli setup-verify-sigma <pk0> <vk0> <pk1> <vk1> <receipt1> [...]
                              # the setup-contribute / setup-verify pair for sigma, the trapdoor of the commitment's proof of
                              # knowledge (reasons: FORMAT, NOT_A_SIGMA_CHANGE, POINT_INVALID, RECEIPT, SCALING, VK); sigma links and
                              # delta links are separate links of a chain
    python -m spp.cli execute target/<name>.json Prover.toml [-o target/<name>.gz]               # `nargo execute`: ACIR witness stack
    python -m spp.cli prove   target/<name>.json target/<name>.gz target/<name>.sppc target/<name>.pk
                              # sunspot's own argument order (acir, witness, constraint system, proving key;
                              # client/proof.helper.ts:58-64): the inputs are taken from the nargo witness file
    python -m spp.cli compile target/<name>.ccs                                                  # the reference's OWN gnark R1CS -> <name>.sppc
    python -m spp.cli setup   target/<name>.ccs [--seed HEX32]                                   # `sunspot setup <ccs>` -> <name>.pk, <name>.vk
    python -m spp.cli prove   target/<name>.json target/<name>.gz target/<name>.ccs target/<name>.pk
                              # `sunspot prove` on the files sunspot itself takes: gnark's solver loop (spp/ccs.py) completes the
                              # witness of the .ccs from the nargo witness, the GPU checks every row, commits and proves

Reference call sites: noir_circuit/prove_linux.sh:66-87, audit_circuit/prove_audit.sh:53-99,
scripts/generate_audit.py:659-691, scripts/benchmark_all.py:646-690 (parses the `nbConstraints=` line).
"""
import argparse
import json
import os
import re
import sys

from . import lib
from .prover import Context, build_circuit, verify

_AUDIT_KEYS = ("c0_packed", "c1_packed", "r", "e1_sparse", "e2", "k0", "k1")
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def _num(tok):
    tok = tok.strip().strip('"')
    return int(tok, 16) if tok.lower().startswith("0x") else int(tok)


def parse_prover_toml(text):
    """Scalars and (possibly multi-line) arrays of quoted hex / bare integers, as written by
    client/proof.helper.ts:32-50 and scripts/generate_audit.py:630-641."""
    out = {}
    for m in re.finditer(r'^(\w+)\s*=\s*(\[[^\]]*\]|[^\n]+)$', text, re.M):
        k, v = m.group(1), m.group(2).strip()
        if v.startswith("["):
            out[k] = [_num(t) for t in re.findall(r'"[^"]*"|-?\w+', v[1:-1])]
        else:
            out[k] = _num(v)
    return out


def input_vector(vals):
    """Circuit input wires (public first) from a parsed Prover.toml; the circuit is recognised by its keys."""
    if "siblings" in vals:
        order = ("root", "nullifier", "recipient", "amount", "wa_commitment", "secret_key", "owner_x", "owner_y", "randomness", "index")
        return lib.SPP_CIRCUIT_WITHDRAW, [vals[k] % R for k in order] + [s % R for s in vals["siblings"]]
    row = [vals["wa_commitment"], vals["ct_commitment"]] + vals["c0_packed"] + vals["c1_packed"] + [vals["secret_key"]]
    for k in ("r", "e1_sparse", "e2", "k0", "k1"):
        row += vals[k]
    return lib.SPP_CIRCUIT_AUDIT, [v % R for v in row]


def _load_partials(paths, pw):
    """the partial files of one record, one per member of one set, as [t, 1, 64, 32] bytes; ValueError otherwise"""
    import numpy as np
    from . import witness
    parts = [witness.load_partial_json(p) for p in paths]
    group = parts[0]["with"]
    if any(q["with"] != group for q in parts) or sorted(q["x"] for q in parts) != group:
        raise ValueError("the partials must be one from every auditor of one set (sets %s, from %s)"
                         % (sorted({tuple(q["with"]) for q in parts}), [q["x"] for q in parts]))
    ct = int.from_bytes(pw[44:76], "big")
    for path, q in zip(paths, parts):
        if q["ct_commitment"] != ct:
            raise ValueError("%s was made for another ciphertext than the one this public witness commits to" % path)
    if len(parts) > 1 and not all(q["masked"] for q in parts):
        print("spp audit-open: warning: unmasked partials -- each of them is a linear equation in its auditor's share", file=sys.stderr)
    return np.stack([q["partial"] for q in parts])[:, None]


def _audit_open(a):
    from . import witness
    try:   # everything that can be wrong with the files is found before a device is opened
        proof, pw = open(a.proof, "rb").read(), open(a.pw, "rb").read()
        if len(proof) != lib.PROOF_LEN or len(pw) != lib.AUDIT_PW_LEN:
            raise ValueError("an audit record is a proof of %d bytes and a public witness of %d" % (lib.PROOF_LEN, lib.AUDIT_PW_LEN))
        shares = partials = None
        if a.partials is not None:
            partials = _load_partials(a.partials, pw)
        else:
            shares = [witness.load_share_json(p) for p in a.shares]
            if len({s["x"] for s in shares}) != len(shares) or len(shares) < max(s["threshold"] for s in shares):
                raise ValueError("need %d shares with distinct indices, got %d" % (max(s["threshold"] for s in shares), len(shares)))
        c0, c1, claimed = witness.load_ciphertext_json(a.ciphertext)
        vk = None if a.vk == "-" else open(a.vk, "rb").read()
    except (OSError, ValueError) as e:
        print("spp audit-open: %s" % e, file=sys.stderr)
        return 2
    ctx = Context(a.device)
    try:
        if partials is not None:
            owners, flags = ctx.audit_open(vk, None, [proof], [pw], [c0], [c1], partials=partials)
        else:
            sk = witness.reconstruct_sk(ctx, shares)
            owners, flags = ctx.audit_open(vk, sk, [proof], [pw], [c0], [c1])
    finally:
        ctx.close()
    f = flags[0]
    print("owner_x = 0x%064x\nowner_y = 0x%064x" % owners[0])
    print("proof: %s" % ("not checked" if vk is None else "FAILED" if f & lib.SPP_AUDIT_BAD_PROOF else "verified"))
    print("ciphertext: %s" % ("NOT the one the proof commits to" if f & lib.SPP_AUDIT_BAD_CIPHERTEXT else "bound to the proof (ct_commitment)"))
    print("identity: %s" % ("NOT the one the proof commits to" if f & lib.SPP_AUDIT_BAD_IDENTITY else "bound to the proof (wa_commitment)"))
    if partials is not None:
        print("partials: %s" % ("do NOT combine to a decryption (a wrong share, set or record)" if f & lib.SPP_AUDIT_BAD_PARTIALS
                                else "combine to a decryption (%d auditors, no key rebuilt)" % len(partials)))
    if claimed is not None and claimed != owners[0]:
        print("note: the prover's expected_owner differs from the decrypted owner")
    return 0 if f == 0 else 1


def _audit_pair_seeds(a):
    from . import witness
    if not 2 <= a.shares <= 255:
        print("spp audit-pair-seeds: need 2 <= shares <= 255", file=sys.stderr)
        return 2
    try:
        os.makedirs(a.out, exist_ok=True)
        seeds = witness.new_pair_seeds(a.shares)
        for i in range(1, a.shares + 1):
            witness.write_pair_seeds_json(os.path.join(a.out, "pair_seeds_%d.json" % i), i, a.shares, seeds[i])
    except OSError as e:
        print("spp audit-pair-seeds: %s" % e, file=sys.stderr)
        return 2
    print("audit-pair-seeds: pair_seeds_1.json .. pair_seeds_%d.json in %s; file i is for auditor i alone" % (a.shares, a.out))
    return 0


def _audit_partial(a):
    from . import witness
    try:   # everything that can be wrong with the files is found before a device is opened
        # `--with 2 3 ciphertext.json a.pw`: the option takes what follows it, the two files included
        others = [int(v) for v in a.others if re.fullmatch(r"\d+", v)]
        rest = [v for v in a.others if not re.fullmatch(r"\d+", v)]
        files = [f for f in (a.ciphertext, a.pw) if f is not None] + rest
        if len(files) != 2:
            raise ValueError("need ciphertext.json and <name>.pw")
        share = witness.load_share_json(a.share)
        xs = [share["x"]] + [x for x in dict.fromkeys(others) if x != share["x"]]
        t = len(xs)
        if min(xs) <= 0 or max(xs) >= 1 << 32 or t > 64:
            raise ValueError("the set is at most 64 distinct share indices in [1, 2^32)")
        if t < share["threshold"]:
            raise ValueError("the key needs %d auditors, the set %s has %d" % (share["threshold"], sorted(xs), t))
        if a.smudge < 0 or t * a.smudge > witness.SMUDGE_BUDGET:
            raise ValueError("--smudge %d with %d auditors: threshold * bound may not exceed 2^17, the ciphertext's own noise needs the rest of "
                             "Delta/2" % (a.smudge, t))
        c0, c1, _ = witness.load_ciphertext_json(files[0])
        pw = open(files[1], "rb").read()
        if len(pw) != lib.AUDIT_PW_LEN:
            raise ValueError("a public witness is %d bytes" % lib.AUDIT_PW_LEN)
        seeds = None
        if a.pair_seeds:
            x, held = witness.load_pair_seeds_json(a.pair_seeds)
            if x != share["x"] or any(j not in held for j in xs[1:]):
                raise ValueError("%s: not the pair seeds of auditor %d with %s" % (a.pair_seeds, share["x"], xs[1:]))
            seeds = [None] + [held[j] for j in xs[1:]]
        elif t > 1:
            print("spp audit-partial: warning: no --pair-seeds: this partial is a linear equation in the share; about 16 of them give it away",
                  file=sys.stderr)
        e, rho = witness.rlwe_sample_smudge(lib.load_library(), 64, a.smudge)
    except (OSError, ValueError, lib.SppError) as e:
        print("spp audit-partial: %s" % e, file=sys.stderr)
        return 2
    ctx = Context(a.device)
    try:
        part, cts = witness.rlwe_partial_decrypt(ctx, xs, 0, share["y"], [c0], [c1], e, rho, seeds, want_commitments=True)
    except lib.SppError as e:
        print("spp audit-partial: %s" % e, file=sys.stderr)
        return 2
    finally:
        ctx.close()
    if cts[0] != int.from_bytes(pw[44:76], "big"):
        print("spp audit-partial: REFUSED: %s is not the ciphertext %s commits to (ct_commitment 0x%064x); nothing written"
              % (files[0], files[1], cts[0]), file=sys.stderr)
        return 1
    with open(a.out, "w") as f:
        json.dump(witness.partial_json(share["x"], xs, cts[0], seeds is not None, a.smudge, part[0]), f, indent=1)
    print("audit-partial: %s: auditor %d within %s, %s, smudged within %d" % (a.out, share["x"], sorted(xs), "masked" if seeds is not None else "UNMASKED", a.smudge))
    return 0


def _load_shares(paths):
    """the share files of a key, enough of them and at distinct indices, or ValueError"""
    from . import witness
    shares = [witness.load_share_json(p) for p in paths]
    need = max(s["threshold"] for s in shares)
    if len({s["x"] for s in shares}) != len(shares) or len(shares) < need:
        raise ValueError("need %d shares with distinct indices, got %d" % (need, len(shares)))
    return shares


def _key_maxima(ctx, pk_a, pk_b, shares):
    from . import witness
    sk = witness.reconstruct_sk(ctx, shares)
    return witness.rlwe_key_check(ctx, pk_a, pk_b, sk)[0]


def _rlwe_keygen(a):
    from . import witness
    t, m = a.threshold, a.shares
    if not (1 <= t <= 64 and t <= m <= 255):
        print("spp rlwe-keygen: need 1 <= threshold <= 64 and threshold <= shares <= 255", file=sys.stderr)
        return 2
    shares_dir = os.path.join(a.out, "rlwe_sk_shares")
    try:
        os.makedirs(shares_dir, exist_ok=True)
    except OSError as e:
        print("spp rlwe-keygen: %s" % e, file=sys.stderr)
        return 2
    bound = witness.NOISE_BOUND
    if a.reference_seed is not None:
        sk, pk_a, e, coeffs = witness.reference_key_draws(a.reference_seed, t)
    else:
        sk, pk_a, e = (x[0] for x in witness.rlwe_sample_key(lib.load_library(), 1, bound))
        coeffs = None                                     # drawn by the library, from the operating system
    pk_path = os.path.join(a.out, "rlwe_pk.json")
    share_paths = [os.path.join(shares_dir, "share_%d.json" % (j + 1)) for j in range(m)]
    ctx = Context(a.device)
    try:
        pk_b, _ = witness.rlwe_keygen(ctx, sk, pk_a, e)
        shares = witness.shamir_split(ctx, [int(v) % R for v in sk], t, m, coeffs=coeffs)
        witness.write_rlwe_pk_json(pk_path, pk_a, pk_b[0])
        witness.write_rlwe_params_json(os.path.join(a.out, "rlwe_params.json"), t, m, bound)
        for j, (path, sh) in enumerate(zip(share_paths, shares)):
            witness.write_share_json(path, j + 1, t, m, sh["x"], sh["y"])
        # the files as a key holder will read them, not the arrays they were written from
        noise, skmax = _key_maxima(ctx, *witness.load_rlwe_pk_json(pk_path), _load_shares(share_paths[:t]))
    except (OSError, ValueError, lib.SppError) as e:
        print("spp rlwe-keygen: %s" % e, file=sys.stderr)
        return 2
    finally:
        ctx.close()
    if noise > bound or skmax > bound:
        print("spp rlwe-keygen: the files in %s FAILED their check (max |b + a*sk| = %d, max |sk| = %d, bound %d): do not use them"
              % (a.out, noise, skmax, bound), file=sys.stderr)
        return 1
    print("rlwe-keygen: %s, rlwe_params.json and %d shares (threshold %d) in %s" % (pk_path, m, t, shares_dir))
    print("check: key reconstructed from shares 1..%d, max |b + a*sk| = %d, max |sk| = %d (bound %d)" % (t, noise, skmax, bound))
    return 0


def _rlwe_key_check(a):
    from . import witness
    try:   # everything that can be wrong with the files is found before a device is opened
        pk_a, pk_b = witness.load_rlwe_pk_json(a.pk)
        shares = _load_shares(a.shares)
        bound = witness.NOISE_BOUND
        params = a.params or os.path.join(os.path.dirname(os.path.abspath(a.pk)), "rlwe_params.json")
        if a.params or os.path.exists(params):
            bound = int(json.load(open(params))["noise_bound"])
    except (OSError, ValueError, KeyError, TypeError) as e:
        print("spp rlwe-key-check: %s" % e, file=sys.stderr)
        return 2
    ctx = Context(a.device)
    try:
        noise, skmax = _key_maxima(ctx, pk_a, pk_b, shares)
    except lib.SppError as e:
        print("spp rlwe-key-check: %s" % e, file=sys.stderr)
        return 2
    finally:
        ctx.close()
    print("max |b + a*sk| = %d\nmax |sk| = %d\nnoise bound = %d" % (noise, skmax, bound))
    ok = noise <= bound and skmax <= bound
    print("key: %s" % ("the shares hold the secret of this public key" if ok else "NOT a key pair within the bound"))
    return 0 if ok else 1


DKG_MAX_SHARES = 10
_DKG_NOISE_PER_KEY, _DKG_SMUDGE_LIMIT, _DKG_HALF_DELTA = 18432, 1 << 17, (167772161 // 256) // 2


def _dkg_refuses_size(cmd, t, m):
    """the message for a committee this command does not serve, or None"""
    if not (1 <= t <= 64 and t <= m <= 255):
        return "spp %s: need 1 <= threshold <= 64 and threshold <= shares <= 255" % cmd
    if m > DKG_MAX_SHARES:
        return ("spp %s: at most %d auditors: a ciphertext under %d summed keys has noise up to %d * %d + 3 = %d, and with the "
                "smudging limit %d that is %d, not below delta / 2 = %d (%d auditors: %d)"
                % (cmd, DKG_MAX_SHARES, m, m, _DKG_NOISE_PER_KEY, m * _DKG_NOISE_PER_KEY + 3, _DKG_SMUDGE_LIMIT,
                   m * _DKG_NOISE_PER_KEY + 3 + _DKG_SMUDGE_LIMIT, _DKG_HALF_DELTA, DKG_MAX_SHARES,
                   DKG_MAX_SHARES * _DKG_NOISE_PER_KEY + 3 + _DKG_SMUDGE_LIMIT))
    return None


def _hex_seed(text):
    seed = bytes.fromhex(text[2:] if text.lower().startswith("0x") else text)
    if len(seed) != 32:
        raise ValueError("--a-seed is 32 bytes in hex")
    return seed


def _dkg_deal(a):
    import hashlib
    from . import witness
    t, m, i = a.threshold, a.shares, a.index
    msg = _dkg_refuses_size("dkg-deal", t, m)
    if msg is None and not 1 <= i <= m:
        msg = "spp dkg-deal: --index is one of the auditors 1..%d" % m
    if msg:
        print(msg, file=sys.stderr)
        return 2
    private = os.path.join(a.out, "private")
    try:
        seed = _hex_seed(a.a_seed)
        os.makedirs(private, exist_ok=True)
    except (OSError, ValueError) as e:
        print("spp dkg-deal: %s" % e, file=sys.stderr)
        return 2
    L = lib.load_library()
    ctx = Context(a.device)
    try:
        deal = {"version": 1, "kind": "refresh" if a.refresh else "key", "index": i, "threshold": t, "num_shares": m, "a_seed": seed.hex()}
        if a.refresh:
            secrets = [0] * witness.RLWE_N
        else:
            sk, _, e = (x[0] for x in witness.rlwe_sample_key(L, 1, witness.NOISE_BOUND))   # its a is not used: a comes from the seed
            pk_b, _ = witness.rlwe_keygen(ctx, sk, witness.dkg_a_from_seed(L, seed), e)
            deal["b"] = ["0x%08x" % int(v) for v in pk_b[0]]
            secrets = [int(v) % R for v in sk]
        d = witness.vss_deal(ctx, secrets, t, m)
        deal["commitments"] = d["commitments"].hex()
        if a.refresh:
            deal["zero_blinds"] = ["%064x" % v for v in d["blinds"]]
        text = json.dumps(deal).encode()
        deal_path = os.path.join(a.out, "deal_%d.json" % i)
        with open(deal_path, "wb") as f:
            f.write(text)
        digest = hashlib.sha256(text).hexdigest()
        with open(os.path.join(a.out, "deal_%d.hash" % i), "w") as f:
            f.write(digest + "\n")
        for sh in d["shares"]:
            with open(os.path.join(private, "subshare_%d_to_%d.json" % (i, sh["x"])), "w") as f:
                json.dump({"from": i, "to": sh["x"], "y": ["%064x" % v for v in sh["y"]], "y_blind": ["%064x" % v for v in sh["y_blind"]]}, f)
    except (OSError, ValueError, lib.SppError) as e:
        print("spp dkg-deal: %s" % e, file=sys.stderr)
        return 2
    finally:
        ctx.close()
    print("dkg-deal: %s (%s, threshold %d of %d) and %d sub-shares in %s" % (deal_path, deal["kind"], t, m, m, private))
    print("publish first: %s" % digest)
    return 0


def _dkg_fail(dealer, check_name, detail):
    print("spp dkg-receive: dealer %d: %s check failed%s" % (dealer, check_name, ": " + detail if detail else ""), file=sys.stderr)
    return 1


def _dkg_receive(a):
    import hashlib
    from . import witness
    j, n = a.index, witness.RLWE_N
    if len(a.hashes) != len(a.deals):
        print("spp dkg-receive: one --hashes file per --deals file, in the same order", file=sys.stderr)
        return 2
    try:   # everything that can be wrong with the files is found before a device is opened
        raw = [open(p, "rb").read() for p in a.deals]
        published = [open(p).read().split()[0].lower() for p in a.hashes]
        subs = [json.load(open(p)) for p in a.subshares]
        old = witness.load_share_json(a.refresh) if a.refresh else None
    except (OSError, ValueError, IndexError) as e:
        print("spp dkg-receive: %s" % e, file=sys.stderr)
        return 2
    deals = {}
    for path, body, want in zip(a.deals, raw, published):
        try:
            d = json.loads(body)
            idx, kind, t, m = int(d["index"]), d["kind"], int(d["threshold"]), int(d["num_shares"])
            if int(d["version"]) != 1 or kind not in ("key", "refresh"):
                raise ValueError("version %r, kind %r" % (d["version"], kind))
            entry = {"kind": kind, "t": t, "m": m, "a_seed": _hex_seed(d["a_seed"]), "commitments": bytes.fromhex(d["commitments"])}
            if kind == "key":
                entry["b"] = [int(v, 16) for v in d["b"]]
                if len(entry["b"]) != n or not all(0 <= v < witness.RLWE_Q for v in entry["b"]):
                    raise ValueError("b is 1024 coefficients in [0, q)")
            else:
                entry["zero_blinds"] = [int(v, 16) for v in d["zero_blinds"]]
                if len(entry["zero_blinds"]) != n:
                    raise ValueError("zero_blinds is 1024 field elements")
        except (KeyError, TypeError, ValueError) as e:
            print("spp dkg-receive: %s: not a deal file (%s)" % (path, e), file=sys.stderr)
            return 2
        if hashlib.sha256(body).hexdigest() != want:
            return _dkg_fail(idx, "hash", "%s is not the file whose SHA-256 was published" % path)
        if idx in deals:
            return _dkg_fail(idx, "missing", "dealt twice")
        deals[idx] = entry
    first = deals[min(deals)] if deals else None
    if first is None:
        print("spp dkg-receive: no deal files", file=sys.stderr)
        return 2
    t, m, kind = first["t"], first["m"], first["kind"]
    msg = _dkg_refuses_size("dkg-receive", t, m)
    if msg is None and not 1 <= j <= m:
        msg = "spp dkg-receive: --index is one of the auditors 1..%d" % m
    if msg is None and (kind == "refresh") != (old is not None):
        msg = "spp dkg-receive: these are %s dealings: %s" % (kind, "give --refresh share_%d.json" % j if old is None else "--refresh takes refresh dealings")
    if msg is None and old is not None and old["x"] != j:
        msg = "spp dkg-receive: %s is the share at x = %d, not auditor %d's" % (a.refresh, old["x"], j)
    if msg:
        print(msg, file=sys.stderr)
        return 2
    for i in range(1, m + 1):
        if i not in deals:
            return _dkg_fail(i, "missing", "no deal file of this dealer among --deals")
        for key, what in (("t", "threshold"), ("m", "num_shares"), ("a_seed", "a_seed"), ("kind", "kind")):
            if deals[i][key] != first[key]:
                return _dkg_fail(i, "agreement", "its %s differs from dealer %d's" % (what, min(deals)))
        if len(deals[i]["commitments"]) != t * n * 64:
            return _dkg_fail(i, "point", "%d commitment bytes, not %d" % (len(deals[i]["commitments"]), t * n * 64))
    if len(deals) != m:
        return _dkg_fail(max(deals), "missing", "not one of the auditors 1..%d" % m)
    ys, yb = {}, {}
    for path, sub in zip(a.subshares, subs):
        try:
            src, dst = int(sub["from"]), int(sub["to"])
            y, b = [int(v, 16) for v in sub["y"]], [int(v, 16) for v in sub["y_blind"]]
        except (KeyError, TypeError, ValueError) as e:
            print("spp dkg-receive: %s: not a sub-share file (%s)" % (path, e), file=sys.stderr)
            return 2
        if dst != j or src in ys or len(y) != n or len(b) != n:
            print("spp dkg-receive: %s: need one sub-share of 1024 values per dealer, addressed to auditor %d" % (path, j), file=sys.stderr)
            return 2
        ys[src], yb[src] = y, b
    for i in range(1, m + 1):
        if i not in ys:
            return _dkg_fail(i, "missing", "no sub-share of this dealer among --subshares")
        for row in (ys[i], yb[i]):
            for v, val in enumerate(row):
                if not 0 <= val < R:
                    return _dkg_fail(i, "share", "value %d is no field element" % v)
        if kind == "refresh":
            for v, val in enumerate(deals[i]["zero_blinds"]):
                if not 0 <= val < R:
                    return _dkg_fail(i, "not-zero", "published blind %d is no field element" % v)
    order = list(range(1, m + 1))
    ctx = Context(a.device)
    try:
        flags, bad, share = witness.vss_receive(ctx, t, j, [deals[i]["commitments"] for i in order], [ys[i] for i in order], [yb[i] for i in order],
                                                zero_blinds=[deals[i]["zero_blinds"] for i in order] if kind == "refresh" else None,
                                                base=old["y"] if old is not None else None)
    except lib.SppError as e:
        print("spp dkg-receive: %s" % e, file=sys.stderr)
        return 2
    finally:
        ctx.close()
    if bad:
        for i, row in zip(order, flags):
            for v, fl in enumerate(row):
                if fl:
                    name = next(nm for bit, nm in witness.VSS_FLAG_NAMES if fl & bit)
                    return _dkg_fail(i, name, "value %d (%d values refused in all)" % (v, bad))
    shares_dir = os.path.join(a.out, "rlwe_sk_shares")
    share_path = os.path.join(shares_dir, "share_%d.json" % j)
    try:
        os.makedirs(shares_dir, exist_ok=True)
        if kind == "key":
            pk_b = [sum(deals[i]["b"][v] for i in order) % witness.RLWE_Q for v in range(n)]
            witness.write_rlwe_pk_json(os.path.join(a.out, "rlwe_pk.json"), witness.dkg_a_from_seed(lib.load_library(), first["a_seed"]), pk_b)
            witness.write_rlwe_params_json(os.path.join(a.out, "rlwe_params.json"), t, m, witness.NOISE_BOUND * m)
        witness.write_share_json(share_path, j, t, m, j, share)
    except (OSError, ValueError, lib.SppError) as e:
        print("spp dkg-receive: %s" % e, file=sys.stderr)
        return 2
    print("dkg-receive: %d dealers, every hash and all %d values of each accepted; %s%s"
          % (m, n, "refreshed " if kind == "refresh" else "rlwe_pk.json, rlwe_params.json and ", share_path))
    return 0


# ---- the committee's commitments and handing the key to a new committee (include/spp.h, the block after spp_vss_receive) ----
_RESHARE_NO_NOISE_LIMIT = ("dkg-deal's limit of %d auditors does not apply here: a reshared key is the same key, so the noise of its "
                           "ciphertexts does not change however many hold it" % DKG_MAX_SHARES)


def _committee_size_refused(cmd, t, m, what="threshold and shares"):
    if not (1 <= t <= 64 and t <= m <= 255):
        return "spp %s: %s: need 1 <= threshold <= 64 and threshold <= shares <= 255" % (cmd, what)
    return None


def _load_committee(path):
    """a committee.json as a dict with bytes for a_seed and commitments; ValueError if it is not one"""
    from . import witness
    try:
        d = json.load(open(path))
        c = {"t": int(d["threshold"]), "m": int(d["num_shares"]), "xs": [int(x) for x in d["xs"]], "a_seed": _hex_seed(d["a_seed"]),
             "commitments": bytes.fromhex(d["commitments"]), "noise_bound": int(d["noise_bound"])}
        if int(d["version"]) != 1:
            raise ValueError("version %r" % d["version"])
    except (KeyError, TypeError, ValueError) as e:
        raise ValueError("%s: not a committee file (%s)" % (path, e))
    if _committee_size_refused("", c["t"], c["m"]) or c["xs"] != list(range(1, c["m"] + 1)) or len(c["commitments"]) != c["t"] * witness.RLWE_N * 64:
        raise ValueError("%s: a committee file holds threshold * 1024 commitments for the auditors 1..num_shares" % path)
    return c


def _write_committee(path, t, m, a_seed, commitments, noise_bound):
    with open(path, "w") as f:
        json.dump({"version": 1, "threshold": t, "num_shares": m, "xs": list(range(1, m + 1)), "a_seed": a_seed.hex(),
                   "noise_bound": int(noise_bound), "commitments": commitments.hex()}, f)


def _load_public_deal(path):
    """the public fields of a deal file of any kind; ValueError if it is not one"""
    try:
        d = json.load(open(path))
        if int(d["version"]) != 1 or d["kind"] not in ("key", "refresh", "reshare"):
            raise ValueError("version %r, kind %r" % (d["version"], d["kind"]))
        out = {"index": int(d["index"]), "kind": d["kind"], "t": int(d["threshold"]), "m": int(d["num_shares"]), "a_seed": _hex_seed(d["a_seed"]),
               "commitments": bytes.fromhex(d["commitments"])}
        if d["kind"] == "reshare":
            out.update({"set": [int(x) for x in d["set"]], "t_new": int(d["new_threshold"]), "m_new": int(d["new_shares"])})
        return out
    except (KeyError, TypeError, ValueError) as e:
        raise ValueError("%s: not a deal file (%s)" % (path, e))


def _fail_named(cmd, who, number, check_name, detail):
    print("spp %s: %s %d: %s check failed%s" % (cmd, who, number, check_name, ": " + detail if detail else ""), file=sys.stderr)
    return 1


def _dkg_committee(a):
    from . import witness
    n = witness.RLWE_N
    try:   # everything that can be wrong with the files is found before a device is opened
        loaded = [_load_public_deal(p) for p in a.deals]
        base = _load_committee(a.base) if a.base else None
    except (OSError, ValueError) as e:
        print("spp dkg-committee: %s" % e, file=sys.stderr)
        return 2
    first = loaded[0]
    t, m, kind = first["t"], first["m"], first["kind"]
    msg = _committee_size_refused("dkg-committee", t, m)
    if msg is None and kind == "reshare":
        msg = "spp dkg-committee: the committee file of a reshared key is written by dkg-reshare-receive"
    if msg is None and (kind == "refresh") != (base is not None):
        msg = "spp dkg-committee: %s" % ("refresh dealings are added to a committee file: give --base" if base is None
                                         else "key dealings make a committee file of their own: --base is for refresh dealings")
    if msg is None and base is not None and (base["t"], base["m"], base["a_seed"]) != (t, m, first["a_seed"]):
        msg = "spp dkg-committee: %s is the committee file of another key or committee" % a.base
    if msg:
        print(msg, file=sys.stderr)
        return 2
    deals = {}
    for d in loaded:
        if d["index"] in deals:
            return _fail_named("dkg-committee", "dealer", d["index"], "missing", "dealt twice")
        deals[d["index"]] = d
    for i in range(1, m + 1):
        if i not in deals:
            return _fail_named("dkg-committee", "dealer", i, "missing", "no deal file of this dealer among --deals")
        for key, what in (("t", "threshold"), ("m", "num_shares"), ("a_seed", "a_seed"), ("kind", "kind")):
            if deals[i][key] != first[key]:
                return _fail_named("dkg-committee", "dealer", i, "agreement", "its %s differs from dealer %d's" % (what, first["index"]))
        if len(deals[i]["commitments"]) != t * n * 64:
            return _fail_named("dkg-committee", "dealer", i, "point", "%d commitment bytes, not %d" % (len(deals[i]["commitments"]), t * n * 64))
    if len(deals) != m:
        return _fail_named("dkg-committee", "dealer", max(deals), "missing", "not one of the auditors 1..%d" % m)
    ctx = Context(a.device)
    try:
        flags, bad, out = witness.vss_combine_commitments(ctx, t, [deals[i]["commitments"] for i in range(1, m + 1)],
                                                          base=base["commitments"] if base else None)
    except lib.SppError as e:
        print("spp dkg-committee: %s" % e, file=sys.stderr)
        return 2
    finally:
        ctx.close()
    if bad:
        for i, row in enumerate(flags, 1):
            for at, fl in enumerate(row):
                if fl:
                    return _fail_named("dkg-committee", "dealer", i, "point", "value %d, coefficient %d (%d commitments refused in all)" % (at % n, at // n, bad))
    try:
        _write_committee(a.out, t, m, first["a_seed"], out, base["noise_bound"] if base else witness.NOISE_BOUND * m)
    except OSError as e:
        print("spp dkg-committee: %s" % e, file=sys.stderr)
        return 2
    print("dkg-committee: %s: the commitments of %d %s dealings%s, threshold %d of %d" % (a.out, m, kind, " added to %s" % a.base if base else "", t, m))
    return 0


def _load_subshare(path, to):
    """(from, y, y_blind) of a sub-share file addressed to auditor `to`; ValueError otherwise"""
    from . import witness
    try:
        sub = json.load(open(path))
        src, dst = int(sub["from"]), int(sub["to"])
        y, b = [int(v, 16) for v in sub["y"]], [int(v, 16) for v in sub["y_blind"]]
    except (KeyError, TypeError, ValueError) as e:
        raise ValueError("%s: not a sub-share file (%s)" % (path, e))
    if dst != to or len(y) != witness.RLWE_N or len(b) != witness.RLWE_N:
        raise ValueError("%s: need a sub-share of 1024 values addressed to auditor %d" % (path, to))
    return src, y, b


def _dkg_reshare_deal(a):
    from . import witness
    T, M = a.new_threshold, a.new_shares
    msg = _committee_size_refused("dkg-reshare-deal", T, M, "--new-threshold and --new-shares")
    if msg is None and not a.blind and not a.subshares:
        msg = "spp dkg-reshare-deal: the blind of the share is needed: --blind blind_J.json, --subshares of every round it was dealt in, or both"
    if msg:
        print(msg, file=sys.stderr)
        return 2
    try:   # everything that can be wrong with the files is found before a device is opened
        share = witness.load_share_json(a.share)
        j = share["x"]
        com = _load_committee(a.committee)
        blind = [0] * witness.RLWE_N
        if a.blind:
            bf = witness.load_share_json(a.blind)
            if bf["x"] != j:
                raise ValueError("%s is the blind at x = %d, not auditor %d's" % (a.blind, bf["x"], j))
            blind = list(bf["y"])
        for path in a.subshares or []:
            _, _, yb = _load_subshare(path, j)
            if not all(0 <= v < R for v in yb):
                raise ValueError("%s: a y_blind is no field element" % path)
            blind = [(x + y) % R for x, y in zip(blind, yb)]
        S = list(a.set)
        if len(S) != com["t"] or len(set(S)) != len(S) or not all(1 <= x <= com["m"] for x in S):
            raise ValueError("--set names exactly the threshold (%d) of distinct old members 1..%d" % (com["t"], com["m"]))
        if j not in S:
            raise ValueError("%s is auditor %d's share, and %d is not in --set" % (a.share, j, j))
    except (OSError, ValueError) as e:
        print("spp dkg-reshare-deal: %s" % e, file=sys.stderr)
        return 2
    ctx = Context(a.device)
    try:
        _, bad, _ = witness.vss_receive(ctx, com["t"], j, [com["commitments"]], [share["y"]], [blind], want_share=False)
        if bad:
            print("spp dkg-reshare-deal: share-mismatch: %d of 1024 values of (share, blind) are not what %s commits auditor %d to; "
                  "the likely cause is a forgotten sub-share file of a refresh round (or a committee file from before it): nothing written"
                  % (bad, a.committee, j), file=sys.stderr)
            return 1
        d = witness.vss_deal(ctx, share["y"], T, M, blinds=blind)
        private = os.path.join(a.out, "private")
        os.makedirs(private, exist_ok=True)
        deal_path = os.path.join(a.out, "reshare_%d.json" % j)
        with open(deal_path, "w") as f:
            json.dump({"version": 1, "kind": "reshare", "index": j, "set": S, "threshold": com["t"], "num_shares": com["m"], "new_threshold": T,
                       "new_shares": M, "a_seed": com["a_seed"].hex(), "commitments": d["commitments"].hex()}, f)
        for sh in d["shares"]:
            with open(os.path.join(private, "subshare_%d_to_%d.json" % (j, sh["x"])), "w") as f:
                json.dump({"from": j, "to": sh["x"], "y": ["%064x" % v for v in sh["y"]], "y_blind": ["%064x" % v for v in sh["y_blind"]]}, f)
    except (OSError, ValueError, lib.SppError) as e:
        print("spp dkg-reshare-deal: %s" % e, file=sys.stderr)
        return 2
    finally:
        ctx.close()
    print("dkg-reshare-deal: %s (old member %d of the set %s, threshold %d of %d -> %d of %d) and %d sub-shares in %s"
          % (deal_path, j, S, com["t"], com["m"], T, M, M, private))
    return 0


def _dkg_reshare_receive(a):
    from . import witness
    k, n, cmd = a.index, witness.RLWE_N, "dkg-reshare-receive"
    try:   # everything that can be wrong with the files is found before a device is opened
        com = _load_committee(a.committee)
        loaded = [_load_public_deal(p) for p in a.deals]
        for path, d in zip(a.deals, loaded):
            if d["kind"] != "reshare":
                raise ValueError("%s is a %s dealing: dkg-reshare-receive takes the reshare_<j>.json files of dkg-reshare-deal" % (path, d["kind"]))
        subs = [_load_subshare(p, k) for p in a.subshares]
    except (OSError, ValueError) as e:
        print("spp %s: %s" % (cmd, e), file=sys.stderr)
        return 2
    first = loaded[0]
    T, M, S = first["t_new"], first["m_new"], first["set"]
    msg = _committee_size_refused(cmd, T, M, "the deals' new_threshold and new_shares")
    if msg is None and not 1 <= k <= M:
        msg = "spp %s: --index is one of the new members 1..%d" % (cmd, M)
    if msg:
        print(msg, file=sys.stderr)
        return 2
    deals = {}
    for d in loaded:
        if d["set"] != S:
            return _fail_named(cmd, "old member", d["index"], "set", "its set %s differs from old member %d's %s" % (d["set"], first["index"], S))
        if d["index"] in deals:
            return _fail_named(cmd, "old member", d["index"], "missing", "dealt twice")
        deals[d["index"]] = d
    if len(S) != com["t"] or len(set(S)) != len(S) or not all(1 <= x <= com["m"] for x in S):
        return _fail_named(cmd, "old member", first["index"], "set", "%s is not exactly the threshold (%d) of distinct old members 1..%d" % (S, com["t"], com["m"]))
    for i in sorted(deals):
        if i not in S:
            return _fail_named(cmd, "old member", i, "set", "not a member of the set %s" % S)
    ys, yb = {}, {}
    for src, y, b in subs:
        ys[src], yb[src] = y, b
    for i in S:
        if i not in deals:
            return _fail_named(cmd, "old member", i, "missing", "no deal file of this member among --deals")
        d = deals[i]
        for got, want, what in ((d["t"], com["t"], "threshold"), (d["m"], com["m"], "num_shares"), (d["a_seed"], com["a_seed"], "a_seed")):
            if got != want:
                return _fail_named(cmd, "old member", i, "agreement", "its %s is not the committee file's" % what)
        for key, what in (("t_new", "new_threshold"), ("m_new", "new_shares")):
            if d[key] != first[key]:
                return _fail_named(cmd, "old member", i, "agreement", "its %s differs from old member %d's" % (what, first["index"]))
        if len(d["commitments"]) != T * n * 64:
            return _fail_named(cmd, "old member", i, "point", "%d commitment bytes, not %d" % (len(d["commitments"]), T * n * 64))
        if i not in ys:
            return _fail_named(cmd, "old member", i, "missing", "no sub-share of this member among --subshares")
        for row in (ys[i], yb[i]):
            for v, val in enumerate(row):
                if not 0 <= val < R:
                    return _fail_named(cmd, "old member", i, "share", "value %d is no field element" % v)
    ctx = Context(a.device)
    try:
        flags, bad, share, blind, out = witness.vss_reshare_receive(ctx, S, T, k, com["commitments"], [deals[i]["commitments"] for i in S],
                                                                    [ys[i] for i in S], [yb[i] for i in S])
    except lib.SppError as e:
        print("spp %s: %s" % (cmd, e), file=sys.stderr)
        return 2
    finally:
        ctx.close()
    if bad:
        for i, row in zip(S, flags):
            for v, fl in enumerate(row):
                if fl:
                    name = next(nm for bit, nm in witness.VSS_RESHARE_FLAG_NAMES if fl & bit)
                    return _fail_named(cmd, "old member", i, name, "value %d (%d values refused in all)" % (v, bad))
    shares_dir, private = os.path.join(a.out, "rlwe_sk_shares"), os.path.join(a.out, "private")
    share_path = os.path.join(shares_dir, "share_%d.json" % k)
    try:
        os.makedirs(shares_dir, exist_ok=True)
        os.makedirs(private, exist_ok=True)
        witness.write_share_json(share_path, k, T, M, k, share)
        witness.write_share_json(os.path.join(private, "blind_%d.json" % k), k, T, M, k, blind)
        _write_committee(os.path.join(a.out, "committee.json"), T, M, com["a_seed"], out, com["noise_bound"])
        witness.write_rlwe_params_json(os.path.join(a.out, "rlwe_params.json"), T, M, com["noise_bound"])
    except (OSError, ValueError) as e:
        print("spp %s: %s" % (cmd, e), file=sys.stderr)
        return 2
    print("dkg-reshare-receive: %d old members, all %d values of each accepted and each constant term the member's own share commitment; "
          "%s, private/blind_%d.json, committee.json (threshold %d of %d) and rlwe_params.json; rlwe_pk.json stays as it is"
          % (len(S), n, share_path, k, T, M))
    return 0


_POOL_FIELDS = {"deposit": (("root", 32),), "submit_audit": (("proof", lib.PROOF_LEN), ("pw", lib.AUDIT_PW_LEN)),
                "withdraw": (("proof", lib.PROOF_LEN), ("pw", lib.WITHDRAW_PW_LEN), ("recipient", 32))}
_POOL_LOG_CHUNK = 1 << 24   # spp_pool_settle_log takes at most 2^24 instructions


def parse_pool_log(lines):
    """[(kind, (bytes, ...))] from the lines of a pool-replay log; raises ValueError naming the line that is not an instruction"""
    out = []
    for no, line in enumerate(lines, 1):
        if not line.strip():
            continue
        try:
            d = json.loads(line)
            (kind, body), = d.items()
            vals = tuple(bytes.fromhex(body[name][2:] if body[name].lower().startswith("0x") else body[name]) for name, _ in _POOL_FIELDS[kind])
        except (ValueError, KeyError, TypeError, AttributeError) as e:
            raise ValueError("line %d: not a deposit / submit_audit / withdraw instruction (%s)" % (no, e))
        for (name, size), v in zip(_POOL_FIELDS[kind], vals):
            if len(v) != size:
                raise ValueError("line %d: %s.%s must be %d bytes, got %d" % (no, kind, name, size, len(v)))
        out.append((kind, vals))
    return out


def parse_pool_commitments(lines, depth=16):
    """The "commitment" a deposit line of a pool-replay log may carry beside "root" (the leaf the deposit appends,
    instructions/deposit.rs:31-36), as ints in log order; None unless EVERY deposit of the log carries one (a log without any is
    replayed as before).  Raises ValueError naming the line: some deposits with and some without, a commitment that is not 32
    bytes or not a canonical field element, more deposits than a tree of `depth` holds."""
    out, without = [], None
    for no, line in enumerate(lines, 1):
        if not line.strip():
            continue
        d = json.loads(line)
        (kind, body), = d.items()
        if kind != "deposit":
            continue
        if "commitment" not in body:
            without = without or no
            continue
        try:
            text = body["commitment"]
            v = bytes.fromhex(text[2:] if text.lower().startswith("0x") else text)
        except (ValueError, TypeError, AttributeError) as e:
            raise ValueError("line %d: deposit.commitment is not a hexadecimal string (%s)" % (no, e))
        if len(v) != 32:
            raise ValueError("line %d: deposit.commitment must be 32 bytes, got %d" % (no, len(v)))
        if int.from_bytes(v, "big") >= R:
            raise ValueError("line %d: deposit.commitment is not a canonical field element" % no)
        out.append(int.from_bytes(v, "big"))
    if not out:
        return None
    if without:
        raise ValueError("line %d: this deposit carries no commitment, others do (all of them or none)" % without)
    if not 1 <= depth <= 32 or len(out) > 1 << depth:
        raise ValueError("%d deposits do not fit a tree of depth %d (1..32)" % (len(out), depth))
    return out


def _print_root_audit(ctx, witness, depth, log, codes, commitments):
    """pool-replay of a log whose deposits carry their commitments: the leaves go into a resident tree, and every line says what
    the program cannot know (it takes new_root as sent, instructions/deposit.rs:31-36,73) -- a deposit whether the root it pushed is
    the root of the leaves so far, an accepted withdraw which size of the leaf list its root belongs to, or `foreign`."""
    with witness.ShieldedPoolMerkleTree(ctx, depth) as tree:
        tree.insert_many(commitments)
        honest = []                                          # honest[k]: the root after deposits 0..k (spp_merkle_tree_prefix_roots)
        for i in range(0, len(commitments), _POOL_LOG_CHUNK):
            honest += tree.prefix_roots(1 + i, min(_POOL_LOG_CHUNK, len(commitments) - i))
        used = [vals[1][12:44] for (kind, vals), c in zip(log, codes) if kind == "withdraw" and c == lib.SPP_POOL_OK]
        sizes = []                                           # of the root words of the accepted withdraws (spp_merkle_tree_find_roots)
        for i in range(0, len(used), _POOL_LOG_CHUNK):
            sizes += tree.find_roots(used[i:i + _POOL_LOG_CHUNK])[0]
    sizes = iter(sizes)
    deposits = differing = accepted = foreign = 0
    for (kind, vals), c in zip(log, codes):
        name = lib.POOL_RESULT_NAMES[c]
        if kind == "deposit":
            same = vals[0] == honest[deposits].to_bytes(32, "big")
            deposits += 1
            differing += not same
            print("%s %s" % (name, "root-of-leaves" if same else "NOT-root-of-leaves"))
        elif kind == "withdraw" and c == lib.SPP_POOL_OK:
            size = next(sizes)
            accepted += 1
            foreign += size is None
            print("%s %s" % (name, "foreign" if size is None else "size %d" % size))
        else:
            print(name)
    print("roots: %d deposits, %d pushed a root that is not the root of the leaves; %d withdraws accepted, %d against a root of no size of the leaves"
          % (deposits, differing, accepted, foreign))


def _pool_replay(a):
    from . import witness
    try:   # everything that can be wrong with the files is found before a device is opened
        wvk, avk = open(a.withdraw_vk, "rb").read(), open(a.audit_vk, "rb").read()
        lines = open(a.log).readlines()
        log = parse_pool_log(lines)
        commitments = parse_pool_commitments(lines, a.depth)
    except (OSError, ValueError) as e:
        print("spp pool-replay: %s" % e, file=sys.stderr)
        return 2
    capacity = a.capacity or max(1, sum(k == "submit_audit" for k, _ in log), sum(k == "withdraw" for k, _ in log))
    ctx = Context(a.device)
    try:
        with witness.Pool(ctx, wvk, avk, capacity, verifier=a.verifier, group=a.group) as pool:
            # the whole log in one call, whatever the interleaving of the kinds (consecutive chunks past 2^24 instructions)
            all_codes = []
            for i in range(0, len(log), _POOL_LOG_CHUNK):
                codes, _ = pool.settle_log([(kind,) + vals for kind, vals in log[i:i + _POOL_LOG_CHUNK]])
                all_codes += codes
                if commitments is None:
                    for c in codes:
                        print(lib.POOL_RESULT_NAMES[c])
            if commitments is not None:
                _print_root_audit(ctx, witness, a.depth, log, all_codes, commitments)
    except lib.SppError as e:
        print("spp pool-replay: %s" % e, file=sys.stderr)
        return 2
    finally:
        ctx.close()
    return 0


def _hex_lines(path, what):
    """the 32-byte values of a file with one hex value per line (0x optional, blank lines skipped); ValueError names the line"""
    out = []
    with open(path) as f:
        for no, line in enumerate(f, 1):
            tok = line.strip()
            if not tok:
                continue
            try:
                v = int(tok, 16)
            except ValueError:
                raise ValueError("%s line %d: not a hexadecimal %s" % (path, no, what))
            if not 0 <= v < 1 << 256:
                raise ValueError("%s line %d: a %s is 32 bytes" % (path, no, what))
            out.append(v)
    return out


def parse_wallet_secrets(text):
    """[(secret_key, amount, randomness)] from the text of a secrets.json; ValueError names the secret the library would refuse"""
    try:
        items = json.loads(text)
        secrets = [tuple(_num(str(d[k])) for k in ("secretKey", "amount", "randomness")) for d in items]
    except (ValueError, KeyError, TypeError) as e:
        raise ValueError("not a list of {secretKey, amount, randomness} (%s)" % e)
    for k, (sk, amount, rnd) in enumerate(secrets):
        if not (0 < sk < R and 0 <= rnd < R):
            raise ValueError("secret %d: secretKey must be in [1, r) and randomness in [0, r)" % k)
        if not 0 <= amount < 1 << 64:
            raise ValueError("secret %d: amount does not fit 64 bits" % k)
    return secrets


def _wallet_sync(a):
    from . import witness
    try:   # everything that can be wrong with the arguments and the files is found before a device is opened
        secrets = parse_wallet_secrets(open(a.secrets).read())
        leaves = _hex_lines(a.leaves, "leaf")
        if any(v >= R for v in leaves):
            raise ValueError("%s: leaf %d is not a canonical field element" % (a.leaves, next(i for i, v in enumerate(leaves) if v >= R)))
        if not 1 <= a.depth <= 32 or len(leaves) > 1 << a.depth:
            raise ValueError("%d leaves do not fit a tree of depth %d (1..32)" % (len(leaves), a.depth))
        if (a.spent or a.audited) and not a.vk:
            raise ValueError("--spent / --audited describe a pool: they need --vk withdraw.vk audit.vk")
        spent = _hex_lines(a.spent, "nullifier") if a.spent else []
        audited = _hex_lines(a.audited, "wa_commitment") if a.audited else []
        wvk, avk = (open(p, "rb").read() for p in a.vk) if a.vk else (None, None)
        recipient = None if a.recipient is None else int(a.recipient, 16)
        if recipient is not None and not 0 <= recipient < R:
            raise ValueError("--recipient is not a canonical field element")
    except (OSError, ValueError) as e:
        print("spp wallet-sync: %s" % e, file=sys.stderr)
        return 2
    hx = lambda v: "0x%064x" % v
    ctx = Context(a.device)
    try:
        with witness.ShieldedPoolMerkleTree(ctx, a.depth) as tree:
            tree.insert_many(leaves)
            pool = witness.Pool(ctx, wvk, avk, max(1, len(spent), len(audited))) if a.vk else None
            try:
                if pool:
                    pool.import_keys(lib.SPP_POOL_NULLIFIERS, spent)
                    pool.import_keys(lib.SPP_POOL_AUDIT_RECORDS, audited)
                records = tree.sync(secrets, pool)
            finally:
                if pool:
                    pool.close()
            root = tree.getRoot()
            _, occurrences = tree.find([r[2] for r in records])
            found = [r[0] for r in records if r[0] is not None]
            siblings = dict(zip(found, tree.getProofs(found)))
    except lib.SppError as e:
        print("spp wallet-sync: %s" % e, file=sys.stderr)
        return 2
    finally:
        ctx.close()
    for (sk, amount, rnd), (index, flags, com, nf, wa, owner), occ in zip(secrets, records, occurrences):
        rec = {"id": hx(com), "secretKey": hx(sk), "publicKeyX": hx(owner[0]), "publicKeyY": hx(owner[1]), "amount": str(amount),
               "randomness": hx(rnd), "commitment": hx(com), "leafIndex": index, "root": hx(root) if index is not None else None,
               "nullifier": hx(nf) if index is not None else None, "waCommitment": hx(wa),
               "siblings": [hx(v) for v in siblings[index]] if index is not None else [],
               "status": "absent" if index is None else "withdrawn" if flags & lib.SPP_WALLET_SPENT else "pending",
               "audited": bool(flags & lib.SPP_WALLET_AUDITED) if a.vk else None, "occurrences": occ}
        if recipient is not None:
            rec["recipient"] = hx(recipient)
        print(json.dumps(rec))
    return 0


def parse_bundle_notes(lines):
    """[(note, address)] from the JSON lines `wallet-sync --recipient` prints: note = (recipient, amount, secret_key, randomness,
    index) as prove_withdrawals takes it, address = the 32 bytes the withdraw instruction names -- the record's "address" (hex) when
    it has one, else the recipient word's 30 bytes and two zero bytes (shielded_pool_program/src/instructions/withdraw.rs:150-154
    compares the first 30).  ValueError names the line: no leaf, no recipient, already withdrawn, a value out of range."""
    out = []
    for no, line in enumerate(lines, 1):
        if not line.strip():
            continue
        try:
            d = json.loads(line)
            sk, amount, rnd = (_num(str(d[k])) for k in ("secretKey", "amount", "randomness"))
            index, recipient = d["leafIndex"], d.get("recipient")
        except (ValueError, KeyError, TypeError) as e:
            raise ValueError("line %d: not a wallet-sync record (%s)" % (no, e))
        if index is None:
            raise ValueError("line %d: the commitment is no leaf (status absent)" % no)
        if recipient is None:
            raise ValueError("line %d: no recipient (run wallet-sync with --recipient)" % no)
        if d.get("status") == "withdrawn":
            raise ValueError("line %d: the note is withdrawn" % no)
        recipient, index = _num(str(recipient)), int(index)
        if not (0 < sk < R and 0 <= rnd < R and 0 <= recipient < 1 << 240 and 0 <= amount < 1 << 64 and 0 <= index < 1 << 32):
            raise ValueError("line %d: secretKey in [1, r), randomness in [0, r), a recipient word of 30 bytes, a 64-bit amount" % no)
        address = bytes.fromhex(d["address"][2:] if d["address"].lower().startswith("0x") else d["address"]) if "address" in d \
            else recipient.to_bytes(30, "big") + bytes(2)
        if len(address) != 32 or int.from_bytes(address[:30], "big") != recipient:
            raise ValueError("line %d: address is not 32 bytes that begin with the recipient word" % no)
        out.append(((recipient, amount, sk, rnd, index), address))
    return out


def _withdraw_bundle(a):
    from . import witness
    from .prover import prove_withdrawals
    try:   # everything that can be wrong with the arguments and the files is found before a device is opened
        pairs = parse_bundle_notes(open(a.notes).readlines())
        if not pairs:
            raise ValueError("%s holds no note" % a.notes)
        pk_a, pk_b = witness.load_rlwe_pk_json(a.rlwe_pk)
        leaves = _hex_lines(a.leaves, "leaf")
        if any(v >= R for v in leaves):
            raise ValueError("%s: leaf %d is not a canonical field element" % (a.leaves, next(i for i, v in enumerate(leaves) if v >= R)))
        if not 1 <= a.depth <= 32 or len(leaves) > 1 << a.depth:
            raise ValueError("%d leaves do not fit a tree of depth %d (1..32)" % (len(leaves), a.depth))
        if a.size is not None and not 0 <= a.size <= len(leaves):
            raise ValueError("--size %d: the leaves file holds %d leaves" % (a.size, len(leaves)))
        if a.audited and not a.vk:
            raise ValueError("--audited describes a pool: it needs --vk withdraw.vk audit.vk")
        audited = _hex_lines(a.audited, "wa_commitment") if a.audited else []
        wvk, avk = (open(p, "rb").read() for p in a.vk) if a.vk else (None, None)
        for p in (a.withdraw_sppc, a.withdraw_pk, a.audit_sppc, a.audit_pk):
            open(p, "rb").close()
        os.makedirs(a.out, exist_ok=True)
    except (OSError, ValueError) as e:
        print("spp withdraw-bundle: %s" % e, file=sys.stderr)
        return 2
    notes, addresses = [n for n, _ in pairs], [ad for _, ad in pairs]
    ctx = Context(a.device)
    hw = ha = pool = None
    try:
        hw = ctx.load_circuit(a.withdraw_sppc, a.withdraw_pk, a.window)
        ha = ctx.load_circuit(a.audit_sppc, a.audit_pk, a.window)
        with witness.ShieldedPoolMerkleTree(ctx, a.depth) as tree:
            tree.insert_many(leaves)
            if audited:
                pool = witness.Pool(ctx, wvk, avk, len(audited))
                pool.import_keys(lib.SPP_POOL_AUDIT_RECORDS, audited)
            bundle = prove_withdrawals(hw, ha, tree, notes, pk_a, pk_b, pool=pool, size=a.size)
            roots = tree.prefix_roots(1, len(leaves)) if a.with_deposits and leaves else []
    except (lib.SppError, ValueError) as e:
        print("spp withdraw-bundle: %s" % e, file=sys.stderr)
        return 2
    finally:
        for h in (pool, hw, ha):
            if h is not None:
                h.close()
        ctx.close()
    with open(os.path.join(a.out, "log.jsonl"), "w") as f:
        for leaf, root in zip(leaves, roots):
            f.write(json.dumps({"deposit": {"root": "%064x" % root, "commitment": "%064x" % leaf}}) + "\n")
        for ins in bundle.log(addresses):
            names = [name for name, _ in _POOL_FIELDS[ins[0]]]
            f.write(json.dumps({ins[0]: {name: v.hex() for name, v in zip(names, ins[1:])}}) + "\n")
    for s in range(bundle.n_audits):
        open(os.path.join(a.out, "record_%d.proof" % s), "wb").write(bundle.audit_proofs[s])
        open(os.path.join(a.out, "record_%d.pw" % s), "wb").write(bundle.audit_pws[s])
        with open(os.path.join(a.out, "ciphertext_%d.json" % s), "w") as f:
            json.dump(witness.ciphertext_json(bundle.c0[s], bundle.c1[s]), f)
    refused = sum(1 for v in bundle.status if v) + sum(1 for v in bundle.audit_status if v)
    print("withdraw-bundle: %d notes, %d audit records (%d identities already audited), %d rows refused; %s" %
          (len(notes), bundle.n_audits, len({n[2] for n, s in zip(notes, bundle.audit_of) if s == lib.SPP_AUDIT_RESIDENT}), refused,
           os.path.join(a.out, "log.jsonl")))
    for i, v in enumerate(bundle.status):
        if v:
            print("note %d: the withdraw circuit refuses it (not the leaf at its index%s)" % (i, "" if a.size is None else " of that size"))
    return 1 if refused else 0


def parse_deposit_records(lines):
    """[(secret_key, amount, randomness)] from the lines of a deposits.jsonl; ValueError names the line the library would refuse"""
    out = []
    for no, line in enumerate(lines, 1):
        if not line.strip():
            continue
        try:
            d = json.loads(line)
            sk, amount, rnd = (_num(str(d[k])) for k in ("secretKey", "amount", "randomness"))
        except (ValueError, KeyError, TypeError) as e:
            raise ValueError("line %d: not a {secretKey, amount, randomness} record (%s)" % (no, e))
        if not (0 < sk < R and 0 <= rnd < R and 0 <= amount < 1 << 64):
            raise ValueError("line %d: secretKey in [1, r), randomness in [0, r), a 64-bit amount" % no)
        out.append((sk, amount, rnd))
    return out


def parse_deposit_log(lines):
    """[(line number, proof, pw, amount)] from the deposit lines of a deposit-prove log, other kinds skipped; ValueError names the line"""
    out = []
    for no, line in enumerate(lines, 1):
        if not line.strip():
            continue
        try:
            d = json.loads(line)
            (kind, body), = d.items()
            if kind != "deposit":
                continue
            unhex = lambda t: bytes.fromhex(t[2:] if t.lower().startswith("0x") else t)
            proof, pw, amount = unhex(body["proof"]), unhex(body["pw"]), _num(str(body["amount"]))
        except (ValueError, KeyError, TypeError, AttributeError) as e:
            raise ValueError("line %d: not a proved deposit {root, commitment, amount, proof, pw} (%s)" % (no, e))
        if len(proof) != lib.PROOF_LEN or len(pw) != lib.DEPOSIT_PW_LEN:
            raise ValueError("line %d: deposit.proof must be %d bytes and deposit.pw %d" % (no, lib.PROOF_LEN, lib.DEPOSIT_PW_LEN))
        if not 0 <= amount < 1 << 64:
            raise ValueError("line %d: deposit.amount does not fit 64 bits" % no)
        out.append((no, proof, pw, amount))
    return out


def _deposit_prove(a):
    from . import witness
    try:   # everything that can be wrong with the arguments and the files is found before a device is opened
        deposits = parse_deposit_records(open(a.deposits).readlines())
        if not deposits:
            raise ValueError("%s holds no deposit" % a.deposits)
        leaves = _hex_lines(a.leaves, "leaf")
        if any(v >= R for v in leaves):
            raise ValueError("%s: leaf %d is not a canonical field element" % (a.leaves, next(i for i, v in enumerate(leaves) if v >= R)))
        if len(leaves) + len(deposits) > 1 << 16:
            raise ValueError("%d leaves and %d deposits do not fit a tree of depth 16" % (len(leaves), len(deposits)))
        for p in (a.sppc, a.pk):
            open(p, "rb").close()
        os.makedirs(a.out, exist_ok=True)
    except (OSError, ValueError) as e:
        print("spp deposit-prove: %s" % e, file=sys.stderr)
        return 2
    ctx = Context(a.device)
    h = None
    try:
        h = ctx.load_circuit(a.sppc, a.pk, a.window)
        with witness.ShieldedPoolMerkleTree(ctx, 16) as tree:
            tree.insert_many(leaves)
            first, commitments, roots, proofs, pws, status = tree.deposit_proved(h, deposits)
    except (lib.SppError, ValueError) as e:
        print("spp deposit-prove: %s" % e, file=sys.stderr)
        return 2
    finally:
        if h is not None:
            h.close()
        ctx.close()
    with open(os.path.join(a.out, "log.jsonl"), "w") as f:
        for k, dep in enumerate(deposits):
            open(os.path.join(a.out, "deposit_%d.proof" % (first + k)), "wb").write(proofs[k])
            open(os.path.join(a.out, "deposit_%d.pw" % (first + k)), "wb").write(pws[k])
            f.write(json.dumps({"deposit": {"root": "%064x" % roots[k], "commitment": "%064x" % commitments[k], "amount": dep[1],
                                            "proof": proofs[k].hex(), "pw": pws[k].hex()}}) + "\n")
    refused = [k for k, v in enumerate(status) if v]
    print("deposit-prove: %d deposits at leaves %d .. %d, %d rows refused; %s" %
          (len(deposits), first, first + len(deposits) - 1, len(refused), os.path.join(a.out, "log.jsonl")))
    for k in refused:
        print("deposit %d: the deposit circuit refuses it" % k)
    return 1 if refused else 0


def _deposit_verify(a):
    from . import witness
    try:   # everything that can be wrong with the files is found before a device is opened
        vk = open(a.vk, "rb").read()
        entries = parse_deposit_log(open(a.log).readlines())
        start_root = None if a.start_root is None else _hex32(a.start_root, "--start-root")
        if a.start_index < 0 or a.start_index >= 1 << 64:
            raise ValueError("--start-index is a leaf count")
    except (OSError, ValueError) as e:
        print("spp deposit-verify: %s" % e, file=sys.stderr)
        return 2
    ctx = Context(a.device)
    try:
        if start_root is None:                       # the empty depth-16 tree (client/merkle.ts:150-156)
            with witness.ShieldedPoolMerkleTree(ctx, 16) as tree:
                start_root = tree.getRoot().to_bytes(32, "big")
        codes = []
        root, index = start_root, a.start_index
        for i in range(0, len(entries), _POOL_LOG_CHUNK):
            part = entries[i:i + _POOL_LOG_CHUNK]
            c, root, index = witness.verify_deposit_chain(ctx, vk, [e[1] for e in part], [e[2] for e in part], root, index,
                                                          lamports=[e[3] for e in part])
            codes += c
    except lib.SppError as e:
        print("spp deposit-verify: %s" % e, file=sys.stderr)
        return 2
    finally:
        ctx.close()
    for c in codes:
        print(lib.DEPOSIT_RESULT_NAMES[c])
    bad = [(e[0], c) for e, c in zip(entries, codes) if c]
    if bad:
        print("spp deposit-verify: line %d: %s (%d of %d deposits not OK)" % (bad[0][0], lib.DEPOSIT_RESULT_NAMES[bad[0][1]], len(bad), len(codes)),
              file=sys.stderr)
        return 1
    return 0


def _verify_batch(a):
    try:   # everything that can be wrong with the files is found before a device is opened
        if not a.files or len(a.files) % 2:
            raise ValueError("verify-batch takes <vk> and then pairs <proof> <pw>")
        vk = open(a.vk, "rb").read()
        proofs = [open(p, "rb").read() for p in a.files[0::2]]
        pws = [open(p, "rb").read() for p in a.files[1::2]]
        if any(len(p) != lib.PROOF_LEN for p in proofs) or len({len(w) for w in pws}) != 1:
            raise ValueError("proofs must be %d bytes and the public witnesses of one length" % lib.PROOF_LEN)
    except (OSError, ValueError) as e:
        print("spp verify-batch: %s" % e, file=sys.stderr)
        return 2
    ctx = Context(a.device)
    try:
        got = ctx.verify_batch_rlc(vk, proofs, pws, group=a.group)
    except lib.SppError as e:
        print("spp verify-batch: %s" % e, file=sys.stderr)
        return 2
    finally:
        ctx.close()
    for path, ok in zip(a.files[0::2], got):
        print("%s: verification %s" % (path, "succeeded" if ok else "FAILED"))
    return 0 if all(got) else 1


def _setup_contribute(a, sigma=False):
    import hashlib
    cmd = "setup-contribute-sigma" if sigma else "setup-contribute"
    try:   # everything that can be wrong with the arguments and the files is found before a device is opened
        entropy = None
        if a.entropy is not None:
            entropy = bytes.fromhex(a.entropy[2:] if a.entropy.lower().startswith("0x") else a.entropy)
            if len(entropy) != 32:
                raise ValueError("--entropy is 32 bytes of hexadecimal")
        for p in (a.pk, a.vk):
            open(p, "rb").close()
        os.makedirs(a.out, exist_ok=True)
    except (OSError, ValueError) as e:
        print("spp %s: %s" % (cmd, e), file=sys.stderr)
        return 2
    name = os.path.splitext(os.path.basename(a.pk))[0]
    pk_out, vk_out, receipt_out = (os.path.join(a.out, name + ext) for ext in (".pk", ".vk", ".receipt"))
    if os.path.exists(pk_out) and os.path.samefile(pk_out, a.pk):
        print("spp %s: --out is the directory of the key itself; the key before is needed to verify the contribution" % cmd, file=sys.stderr)
        return 2
    ctx = Context(a.device)
    try:
        receipt = (ctx.setup_contribute_sigma if sigma else ctx.setup_contribute)(a.pk, a.vk, pk_out, vk_out, entropy)
    except lib.SppError as e:
        print("spp %s: %s" % (cmd, e), file=sys.stderr)
        return 2
    finally:
        ctx.close()
    open(receipt_out, "wb").write(receipt)
    print("%s: %s, %s" % (cmd, pk_out, vk_out))
    print("receipt %s sha256 %s" % (receipt_out, hashlib.sha256(receipt).hexdigest()))
    return 0


def parse_ceremony_chain(files):
    """[(pk_before, vk_before, pk_after, vk_after, receipt path)] per link from the arguments of setup-verify, or ValueError"""
    if len(files) < 5 or (len(files) - 2) % 3:
        raise ValueError("setup-verify takes <pk0> <vk0> and then triples <pk> <vk> <receipt>")
    keys = [(files[0], files[1])] + [(files[i], files[i + 1]) for i in range(2, len(files), 3)]
    return [keys[k] + keys[k + 1] + (files[4 + 3 * k],) for k in range(len(keys) - 1)]


def _setup_verify(a, sigma=False):
    cmd = "setup-verify-sigma" if sigma else "setup-verify"
    names = lib.SIGMA_REASON_NAMES if sigma else lib.CONTRIB_REASON_NAMES
    try:   # everything that can be wrong with the arguments and the files is found before a device is opened
        links = parse_ceremony_chain(a.files)
        for p in a.files:
            open(p, "rb").close()
        receipts = [open(link[4], "rb").read() for link in links]
    except (OSError, ValueError) as e:
        print("spp %s: %s" % (cmd, e), file=sys.stderr)
        return 2
    ctx = Context(a.device)
    try:
        for k, (link, receipt) in enumerate(zip(links, receipts), 1):
            if len(receipt) != lib.SPP_CONTRIB_RECEIPT_LEN:
                ok, reason = False, lib.SPP_CONTRIB_FORMAT
            else:
                ok, reason = (ctx.setup_verify_sigma_contribution if sigma else ctx.setup_verify_contribution)(*link[:4], receipt)
            if not ok:
                print("link %d (%s): REFUSED, %s" % (k, link[2], names[reason]))
                return 1
            print("link %d (%s): a contribution to %s" % (k, link[2], link[0]))
    except lib.SppError as e:
        print("spp %s: %s" % (cmd, e), file=sys.stderr)
        return 2
    finally:
        ctx.close()
    print("%s: %d links verified" % (cmd, len(links)))
    return 0


def _hex32(text, what):
    raw = bytes.fromhex(text[2:] if text.lower().startswith("0x") else text)
    if len(raw) != 32:
        raise ValueError("%s is 32 bytes of hexadecimal" % what)
    return raw


def _setup_derive(a):
    try:
        for p in (a.sppc, a.ptau):
            open(p, "rb").close()
        os.makedirs(a.out, exist_ok=True)
    except OSError as e:
        print("spp setup-derive: %s" % e, file=sys.stderr)
        return 2
    name = os.path.splitext(os.path.basename(a.sppc))[0]
    pk, vk = (os.path.join(a.out, name + ext) for ext in (".pk", ".vk"))
    ctx = Context(a.device)
    try:
        ctx.setup_from_ptau(a.sppc, a.ptau, pk, vk)
    except lib.SppError as e:
        print("spp setup-derive: %s" % e, file=sys.stderr)
        return 2
    finally:
        ctx.close()
    print("setup-derive: %s, %s (gamma = delta = sigma = 1: contribute to delta and sigma next)" % (pk, vk))
    return 0


def _ptau_new(a):
    try:
        if not 1 <= a.log <= 20:
            raise ValueError("the domain's logarithm is in [1, 20]")
        lib.check(lib.load_library().spp_ptau_new(a.log, a.out.encode()))   # host only: no device is opened
    except (ValueError, lib.SppError) as e:
        print("spp ptau-new: %s" % e, file=sys.stderr)
        return 2
    print("ptau-new: %s (tau = alpha = beta = 1, domains up to 2^%d)" % (a.out, a.log))
    return 0


def _ptau_contribute(a):
    import hashlib
    try:   # everything that can be wrong with the arguments and the files is found before a device is opened
        entropy = None if a.entropy is None else _hex32(a.entropy, "--entropy")
        open(a.ptau, "rb").close()
        os.makedirs(a.out, exist_ok=True)
    except (OSError, ValueError) as e:
        print("spp ptau-contribute: %s" % e, file=sys.stderr)
        return 2
    name = os.path.splitext(os.path.basename(a.ptau))[0]
    out, receipt_out = (os.path.join(a.out, name + ext) for ext in (".ptau", ".receipt"))
    if os.path.exists(out) and os.path.samefile(out, a.ptau):
        print("spp ptau-contribute: --out is the directory of the transcript itself; the transcript before is needed to verify the contribution",
              file=sys.stderr)
        return 2
    ctx = Context(a.device)
    try:
        receipt = ctx.ptau_contribute(a.ptau, out, entropy)
    except lib.SppError as e:
        print("spp ptau-contribute: %s" % e, file=sys.stderr)
        return 2
    finally:
        ctx.close()
    open(receipt_out, "wb").write(receipt)
    print("ptau-contribute: %s" % out)
    print("receipt %s sha256 %s" % (receipt_out, hashlib.sha256(receipt).hexdigest()))
    return 0


def parse_ptau_chain(files):
    """[(transcript before, transcript after, receipt path)] per link from the arguments of ptau-verify, or ValueError"""
    if len(files) < 3 or (len(files) - 1) % 2:
        raise ValueError("ptau-verify takes <t0> and then pairs <transcript> <receipt>")
    return [(files[0] if k == 0 else files[2 * k - 1], files[2 * k + 1], files[2 * k + 2]) for k in range((len(files) - 1) // 2)]


def _ptau_verify(a):
    try:   # everything that can be wrong with the arguments and the files is found before a device is opened
        links = parse_ptau_chain(a.files)
        for p in a.files:
            open(p, "rb").close()
        receipts = [open(link[2], "rb").read() for link in links]
    except (OSError, ValueError) as e:
        print("spp ptau-verify: %s" % e, file=sys.stderr)
        return 2
    ctx = Context(a.device)
    try:
        for k, (link, receipt) in enumerate(zip(links, receipts), 1):
            if len(receipt) != lib.SPP_PTAU_RECEIPT_LEN:
                ok, reason = False, lib.SPP_PTAU_FORMAT
            else:
                ok, reason = ctx.ptau_verify_contribution(link[0], link[1], receipt)
            if not ok:
                print("link %d (%s): REFUSED, %s" % (k, link[1], lib.PTAU_REASON_NAMES[reason]))
                return 1
            print("link %d (%s): a contribution to %s" % (k, link[1], link[0]))
    except lib.SppError as e:
        print("spp ptau-verify: %s" % e, file=sys.stderr)
        return 2
    finally:
        ctx.close()
    print("ptau-verify: %d links verified" % len(links))
    return 0


def main(argv=None):
    ap = argparse.ArgumentParser(prog="spp")
    sub = ap.add_subparsers(dest="cmd", required=True)
    c = sub.add_parser("compile"); c.add_argument("circuit", help="withdraw | audit | deposit | path of a nargo-compiled target/<name>.json (ACIR)")
    c.add_argument("--rlwe-pk"); c.add_argument("-o", "--out", default=None)
    s = sub.add_parser("setup"); s.add_argument("sppc"); s.add_argument("--seed", default=None); s.add_argument("--device", type=int, default=0)
    s.add_argument("--force", action="store_true", help="redo the setup even when matching keys exist")
    p = sub.add_parser("prove"); p.add_argument("files", nargs="+", help="<sppc> <pk> <Prover.toml>  |  <acir.json> <witness.gz> <sppc> <pk>")
    p.add_argument("--device", type=int, default=0)
    p.add_argument("--window", type=int, default=0)
    p.add_argument("--rs", nargs=2, default=None, metavar=("R", "S"),
                   help="blinding factors (parity runs only: the default draws fresh ones from the OS, as every real proof must)")
    x = sub.add_parser("execute"); x.add_argument("acir"); x.add_argument("toml"); x.add_argument("-o", "--out", default=None)
    v = sub.add_parser("verify"); v.add_argument("vk"); v.add_argument("proof"); v.add_argument("pw")
    vb = sub.add_parser("verify-batch"); vb.add_argument("vk"); vb.add_argument("files", nargs="+", metavar="PROOF PW")
    vb.add_argument("--group", type=int, default=0, help="proofs per combined equation (a multiple of 64 in [64, 4096]; default 256)")
    vb.add_argument("--device", type=int, default=0)
    o = sub.add_parser("audit-open"); o.add_argument("vk", help="verifying key, or - for a record already verified elsewhere")
    o.add_argument("proof"); o.add_argument("pw"); o.add_argument("ciphertext", help="ciphertext.json (scripts/generate_audit.py:590-606)")
    og = o.add_mutually_exclusive_group(required=True)
    og.add_argument("--shares", nargs="+", default=None, metavar="SHARE.json", help="threshold many share files (scripts/rlwe_keygen.py)")
    og.add_argument("--partials", nargs="+", default=None, metavar="PARTIAL.json", help="instead of --shares: one audit-partial file per auditor of one set")
    o.add_argument("--device", type=int, default=0)
    ps = sub.add_parser("audit-pair-seeds"); ps.add_argument("--shares", type=int, required=True, metavar="M"); ps.add_argument("--out", required=True, metavar="DIR")
    pa = sub.add_parser("audit-partial"); pa.add_argument("share", help="this auditor's share_<i>.json")
    pa.add_argument("ciphertext", nargs="?", default=None); pa.add_argument("pw", nargs="?", default=None)
    pa.add_argument("--with", dest="others", nargs="+", default=[], metavar="X", help="the share indices of the other auditors of the set")
    pa.add_argument("--pair-seeds", default=None, metavar="pair_seeds_<i>.json")
    pa.add_argument("--smudge", type=int, default=1024, metavar="B", help="noise bound per slot (default 1024; threshold * B <= 2^17)")
    pa.add_argument("--out", required=True, metavar="partial_<i>.json"); pa.add_argument("--device", type=int, default=0)
    r = sub.add_parser("pool-replay"); r.add_argument("withdraw_vk"); r.add_argument("audit_vk"); r.add_argument("log", help="one instruction per line (JSON)")
    r.add_argument("--capacity", type=int, default=0, help="keys per set (default: enough for the log)")
    r.add_argument("--verifier", choices=("each", "rlc"), default="each", help="each: one lane per proof (default); rlc: random linear combination")
    r.add_argument("--group", type=int, default=0, help="with --verifier rlc: proofs per combined equation (a multiple of 64 in [64, 4096]; default 256)")
    r.add_argument("--depth", type=int, default=16, help="of the tree the deposits' commitments go into, when the log carries them")
    r.add_argument("--device", type=int, default=0)
    w = sub.add_parser("wallet-sync"); w.add_argument("secrets", help="JSON list of {secretKey, amount, randomness}")
    w.add_argument("leaves", help="one hex leaf per line, in chain order")
    w.add_argument("--spent", default=None, metavar="NULLIFIERS.txt", help="spent nullifiers, one hex key per line (needs --vk)")
    w.add_argument("--audited", default=None, metavar="WA.txt", help="wa_commitments with an audit record, one hex key per line (needs --vk)")
    w.add_argument("--vk", nargs=2, default=None, metavar=("WITHDRAW.vk", "AUDIT.vk"))
    w.add_argument("--recipient", default=None, metavar="HEX", help="recipient word copied into every record")
    w.add_argument("--depth", type=int, default=16); w.add_argument("--device", type=int, default=0)
    wb = sub.add_parser("withdraw-bundle"); wb.add_argument("notes", help="the JSON lines of `wallet-sync --recipient`")
    wb.add_argument("withdraw_sppc"); wb.add_argument("withdraw_pk"); wb.add_argument("audit_sppc"); wb.add_argument("audit_pk")
    wb.add_argument("rlwe_pk", help="rlwe_pk.json"); wb.add_argument("leaves", help="one hex leaf per line, in chain order")
    wb.add_argument("--out", required=True, metavar="DIR", help="log.jsonl, record_<s>.proof / .pw and ciphertext_<s>.json go here")
    wb.add_argument("--audited", default=None, metavar="WA.txt", help="wa_commitments with an audit record, one hex key per line (needs --vk)")
    wb.add_argument("--vk", nargs=2, default=None, metavar=("WITHDRAW.vk", "AUDIT.vk"))
    wb.add_argument("--size", type=int, default=None, help="prove against the tree of the first SIZE leaves (a root the pool still holds)")
    wb.add_argument("--with-deposits", action="store_true", help="begin the log with one deposit line per leaf, so that it replays on a fresh pool")
    wb.add_argument("--window", type=int, default=0); wb.add_argument("--depth", type=int, default=16); wb.add_argument("--device", type=int, default=0)
    dp = sub.add_parser("deposit-prove"); dp.add_argument("deposits", help="one {secretKey, amount, randomness} per line (JSON)")
    dp.add_argument("sppc"); dp.add_argument("pk"); dp.add_argument("leaves", help="the leaves so far, one hex leaf per line, in chain order")
    dp.add_argument("--out", required=True, metavar="DIR", help="log.jsonl and deposit_<i>.proof / .pw go here")
    dp.add_argument("--window", type=int, default=0); dp.add_argument("--device", type=int, default=0)
    dv = sub.add_parser("deposit-verify"); dv.add_argument("vk"); dv.add_argument("log", help="the log.jsonl of deposit-prove")
    dv.add_argument("--start-root", default=None, metavar="HEX", help="the root before the first line (default: the empty depth-16 tree)")
    dv.add_argument("--start-index", type=int, default=0, metavar="N", help="the leaf count before the first line")
    dv.add_argument("--device", type=int, default=0)
    k = sub.add_parser("rlwe-keygen"); k.add_argument("--out", required=True, metavar="DIR")
    k.add_argument("--threshold", type=int, default=2); k.add_argument("--shares", type=int, default=3)
    k.add_argument("--reference-seed", type=int, default=None, metavar="N",
                   help="draw from random.Random(N) in the order of scripts/rlwe_keygen.py: for reproducing fixtures only, "
                        "NEVER a key to use (the default is the operating system's randomness)")
    k.add_argument("--device", type=int, default=0)
    kc = sub.add_parser("rlwe-key-check"); kc.add_argument("pk", help="rlwe_pk.json")
    kc.add_argument("--shares", nargs="+", required=True, metavar="SHARE.json", help="threshold many share files")
    kc.add_argument("--params", default=None, help="rlwe_params.json (default: next to the public key; without one the bound is 3)")
    kc.add_argument("--device", type=int, default=0)
    dd = sub.add_parser("dkg-deal"); dd.add_argument("--index", type=int, required=True, metavar="I", help="this auditor, 1..M")
    dd.add_argument("--threshold", type=int, required=True); dd.add_argument("--shares", type=int, required=True, metavar="M")
    dd.add_argument("--a-seed", required=True, metavar="HEX32", help="the seed of the common a, agreed beforehand")
    dd.add_argument("--out", required=True, metavar="DIR"); dd.add_argument("--refresh", action="store_true", help="deal zeros: renews shares, keeps the key")
    dd.add_argument("--device", type=int, default=0)
    dr = sub.add_parser("dkg-receive"); dr.add_argument("--index", type=int, required=True, metavar="J", help="this auditor, 1..M")
    dr.add_argument("--deals", nargs="+", required=True, metavar="DEAL.json"); dr.add_argument("--hashes", nargs="+", required=True, metavar="DEAL.hash")
    dr.add_argument("--subshares", nargs="+", required=True, metavar="SUBSHARE.json"); dr.add_argument("--out", required=True, metavar="DIR")
    dr.add_argument("--refresh", default=None, metavar="SHARE.json", help="this auditor's current share: the dealings are refresh dealings")
    dr.add_argument("--device", type=int, default=0)
    dc = sub.add_parser("dkg-committee", description="The committee's commitments from the public deal files: holds no secrets.")
    dc.add_argument("--deals", nargs="+", required=True, metavar="DEAL.json", help="one deal file per auditor, all key or all refresh dealings")
    dc.add_argument("--base", default=None, metavar="COMMITTEE.json", help="refresh dealings: the committee file they are added to")
    dc.add_argument("--out", required=True, metavar="COMMITTEE.json"); dc.add_argument("--device", type=int, default=0)
    rd = sub.add_parser("dkg-reshare-deal", description="An old member deals its share to a new committee. " + _RESHARE_NO_NOISE_LIMIT + ".")
    rd.add_argument("--share", required=True, metavar="SHARE_J.json")
    rd.add_argument("--blind", default=None, metavar="BLIND_J.json", help="the blind a dkg-reshare-receive wrote")
    rd.add_argument("--subshares", nargs="+", default=None, metavar="SUBSHARE.json",
                    help="every sub-share file addressed to this auditor since the key round (or since --blind): their y_blind sum to the blind")
    rd.add_argument("--committee", required=True, metavar="COMMITTEE.json")
    rd.add_argument("--set", nargs="+", type=int, required=True, metavar="X", help="the old members who deal: exactly the old threshold")
    rd.add_argument("--new-threshold", type=int, required=True, metavar="T", help="1 <= T <= 64")
    rd.add_argument("--new-shares", type=int, required=True, metavar="M", help="T <= M <= 255; " + _RESHARE_NO_NOISE_LIMIT)
    rd.add_argument("--out", required=True, metavar="DIR"); rd.add_argument("--device", type=int, default=0)
    rr = sub.add_parser("dkg-reshare-receive"); rr.add_argument("--index", type=int, required=True, metavar="K", help="this new member, 1..M")
    rr.add_argument("--committee", required=True, metavar="COMMITTEE.json", help="the old committee's file")
    rr.add_argument("--deals", nargs="+", required=True, metavar="RESHARE.json"); rr.add_argument("--subshares", nargs="+", required=True, metavar="SUBSHARE.json")
    rr.add_argument("--out", required=True, metavar="DIR"); rr.add_argument("--device", type=int, default=0)
    sc = sub.add_parser("setup-contribute"); sc.add_argument("pk"); sc.add_argument("vk")
    sc.add_argument("--out", required=True, metavar="DIR", help="<name>.pk, <name>.vk and <name>.receipt go here (not the key's own directory)")
    sc.add_argument("--entropy", default=None, metavar="HEX32", help="for reproducible tests only: the default draws from the operating system")
    sc.add_argument("--device", type=int, default=0)
    sv = sub.add_parser("setup-verify"); sv.add_argument("files", nargs="+", metavar="FILE", help="<pk0> <vk0> then <pk> <vk> <receipt> per link")
    sv.add_argument("--device", type=int, default=0)
    pn = sub.add_parser("ptau-new"); pn.add_argument("log", type=int, help="domains up to 2^log"); pn.add_argument("--out", required=True, metavar="FILE")
    pc = sub.add_parser("ptau-contribute"); pc.add_argument("ptau")
    pc.add_argument("--out", required=True, metavar="DIR", help="<name>.ptau and <name>.receipt go here (not the transcript's own directory)")
    pc.add_argument("--entropy", default=None, metavar="HEX32", help="for reproducible tests only: the default draws from the operating system")
    pc.add_argument("--device", type=int, default=0)
    pv = sub.add_parser("ptau-verify"); pv.add_argument("files", nargs="+", metavar="FILE", help="<t0> then <transcript> <receipt> per link")
    pv.add_argument("--device", type=int, default=0)
    sd = sub.add_parser("setup-derive"); sd.add_argument("sppc"); sd.add_argument("ptau")
    sd.add_argument("--out", required=True, metavar="DIR", help="<name>.pk and <name>.vk go here"); sd.add_argument("--device", type=int, default=0)
    ss = sub.add_parser("setup-contribute-sigma"); ss.add_argument("pk"); ss.add_argument("vk")
    ss.add_argument("--out", required=True, metavar="DIR", help="<name>.pk, <name>.vk and <name>.receipt go here (not the key's own directory)")
    ss.add_argument("--entropy", default=None, metavar="HEX32", help="for reproducible tests only: the default draws from the operating system")
    ss.add_argument("--device", type=int, default=0)
    sw = sub.add_parser("setup-verify-sigma"); sw.add_argument("files", nargs="+", metavar="FILE", help="<pk0> <vk0> then <pk> <vk> <receipt> per link")
    sw.add_argument("--device", type=int, default=0)
    a = ap.parse_args(argv)
    if a.cmd == "setup-derive":
        return _setup_derive(a)
    if a.cmd == "setup-contribute-sigma":
        return _setup_contribute(a, sigma=True)
    if a.cmd == "setup-verify-sigma":
        return _setup_verify(a, sigma=True)
    if a.cmd == "ptau-new":
        return _ptau_new(a)
    if a.cmd == "ptau-contribute":
        return _ptau_contribute(a)
    if a.cmd == "ptau-verify":
        return _ptau_verify(a)
    if a.cmd == "setup-contribute":
        return _setup_contribute(a)
    if a.cmd == "setup-verify":
        return _setup_verify(a)
    if a.cmd == "dkg-deal":
        return _dkg_deal(a)
    if a.cmd == "dkg-receive":
        return _dkg_receive(a)
    if a.cmd == "dkg-committee":
        return _dkg_committee(a)
    if a.cmd == "dkg-reshare-deal":
        return _dkg_reshare_deal(a)
    if a.cmd == "dkg-reshare-receive":
        return _dkg_reshare_receive(a)
    if a.cmd == "rlwe-keygen":
        return _rlwe_keygen(a)
    if a.cmd == "rlwe-key-check":
        return _rlwe_key_check(a)
    if a.cmd == "audit-open":
        return _audit_open(a)
    if a.cmd == "audit-pair-seeds":
        return _audit_pair_seeds(a)
    if a.cmd == "audit-partial":
        return _audit_partial(a)
    if a.cmd == "verify-batch":
        return _verify_batch(a)
    if a.cmd == "pool-replay":
        return _pool_replay(a)
    if a.cmd == "wallet-sync":
        return _wallet_sync(a)
    if a.cmd == "withdraw-bundle":
        return _withdraw_bundle(a)
    if a.cmd == "deposit-prove":
        return _deposit_prove(a)
    if a.cmd == "deposit-verify":
        return _deposit_verify(a)
    if a.cmd == "compile" and a.circuit.endswith(".ccs"):
        from . import ccs
        c = ccs.load_ccs(a.circuit)
        n = ccs.to_sppc(ccs.decode_system(c), c, a.out or os.path.splitext(a.circuit)[0] + ".sppc")
        print("nbConstraints=%d" % n)
        return 0
    if a.cmd == "setup" and a.sppc.endswith(".ccs"):
        from . import ccs
        c = ccs.load_ccs(a.sppc)
        a.sppc = os.path.splitext(a.sppc)[0] + ".sppc"
        ccs.to_sppc(ccs.decode_system(c), c, a.sppc)
    if a.cmd == "compile":
        if a.circuit not in ("withdraw", "audit", "deposit"):
            # `sunspot compile target/<name>.json` (prove_linux.sh:66-70): the reference's own compiled ACIR -> R1CS
            from . import acir
            out = a.out or os.path.splitext(a.circuit)[0] + ".sppc"
            try:
                n = acir.compile_to_sppc(a.circuit, out)
            except (acir.AcirFormatError, lib.SppError) as e:
                print("spp compile: %s" % e, file=sys.stderr)
                return 1
            print("nbConstraints=%d" % n)
            return 0
        if not a.out:
            ap.error("-o/--out is required")
        aux = None
        if a.circuit == "audit":
            if not a.rlwe_pk:
                ap.error("audit needs --rlwe-pk (demo-frontend/public/rlwe/rlwe_pk.json)")
            pk = json.load(open(a.rlwe_pk))
            aux = [_num(str(x)) for x in pk["a"]] + [_num(str(x)) for x in pk["b"]]
        n = build_circuit({"withdraw": lib.SPP_CIRCUIT_WITHDRAW, "audit": lib.SPP_CIRCUIT_AUDIT, "deposit": lib.SPP_CIRCUIT_DEPOSIT}[a.circuit], a.out, aux)
        print("nbConstraints=%d" % n)
        return 0
    if a.cmd == "setup":
        # the skip-if-exists step of noir_circuit/prove_linux.sh:72-79 ("if [ ! -f pk ] || [ ! -f vk ]; then sunspot setup"),
        # made safe: the keys are reused only when <name>.setup.json records the hash of THIS circuit file (and the same
        # seed, when one is given); a circuit rebuilt with other constraints gets a fresh setup.
        import hashlib
        base = os.path.splitext(a.sppc)[0]
        meta_path = base + ".setup.json"
        digest = hashlib.sha256(open(a.sppc, "rb").read()).hexdigest()
        if not a.force and all(os.path.exists(base + e) for e in (".pk", ".vk")) and os.path.exists(meta_path):
            try:
                meta = json.load(open(meta_path))
            except Exception:
                meta = {}
            if meta.get("circuit_sha256") == digest and (a.seed is None or meta.get("seed_sha256") == hashlib.sha256(bytes.fromhex(a.seed)).hexdigest()) \
                    and meta.get("pk_bytes") == os.path.getsize(base + ".pk"):
                print("setup: %s.pk / .vk are up to date for this circuit (use --force to redo)" % base)
                return 0
        seed = bytes.fromhex(a.seed) if a.seed else os.urandom(32)
        ctx = Context(a.device)
        ctx.setup(a.sppc, seed, base + ".pk", base + ".vk")
        ctx.close()
        json.dump({"circuit_sha256": digest, "seed_sha256": hashlib.sha256(seed).hexdigest(), "pk_bytes": os.path.getsize(base + ".pk")},
                  open(meta_path, "w"))
        return 0
    if a.cmd == "execute":
        from . import acir
        prog = acir.load_program(a.acir)
        _, row = input_vector(parse_prover_toml(open(a.toml).read()))
        try:
            w = acir.execute(prog, row)
        except acir.UnsatisfiedConstraint as e:
            print("spp execute: %s" % e, file=sys.stderr)
            return 1
        out = a.out or os.path.splitext(a.acir)[0] + ".gz"
        acir.write_witness_stack(out, w)
        print("[%s] Circuit witness successfully solved" % prog.main.name)
        print("[%s] Witness saved to %s" % (prog.main.name, out))
        return 0
    if a.cmd == "prove":
        if len(a.files) == 3:
            sppc, pk, toml = a.files
            _, row = input_vector(parse_prover_toml(open(toml).read()))
        elif len(a.files) == 4 and a.files[2].endswith(".ccs"):
            # the reference's own constraint system: every wire is an input of the container, the witness comes from gnark's
            # solver loop over the decoded .ccs, fed with the nargo witness and the commitment challenge of THIS proving key
            from . import acir, ccs
            acir_path, gz, ccs_path, pk = a.files
            c = ccs.load_ccs(ccs_path)
            system = ccs.decode_system(c)
            sppc = os.path.splitext(ccs_path)[0] + ".sppc"
            ccs.to_sppc(system, c, sppc)          # always from THIS .ccs: a stale container of another system must not be proved
            stack = acir.read_witness_stack(gz)
            public = acir.abi_input_row(acir.load_program(acir_path), stack)[:len(c.public) - 1]
            secret = {"__witness_%d" % k: v for k, v in stack.items()}
            ctx = Context(a.device)
            h = ctx.load_circuit(sppc, pk, a.window)
            try:
                row = ccs.reference_witness(system, c, public, secret, lambda partial: h.commitment_challenge([partial])[0])
                proofs, pws, status = h.prove_batch([row])
            except (ValueError, KeyError) as e:
                print("spp prove: %s" % e, file=sys.stderr)
                return 1
            finally:
                h.close()
                ctx.close()
            if status[0] != 0:
                print("spp prove: inputs do not satisfy the circuit", file=sys.stderr)
                return 1
            base = os.path.splitext(ccs_path)[0]
            open(base + ".proof", "wb").write(proofs[0])
            open(base + ".pw", "wb").write(pws[0])
            return 0
        elif len(a.files) == 4:
            from . import acir
            acir_path, gz, sppc, pk = a.files
            row = acir.abi_input_row(acir.load_program(acir_path), acir.read_witness_stack(gz))
        else:
            ap.error("prove takes <sppc> <pk> <Prover.toml> or <acir.json> <witness.gz> <sppc> <pk>")
        a.sppc, a.pk = sppc, pk
        base = os.path.splitext(a.sppc)[0]
        ctx = Context(a.device)
        h = ctx.load_circuit(a.sppc, a.pk, a.window)
        proofs, pws, status = h.prove_batch([row], None if a.rs is None else [(_num(a.rs[0]), _num(a.rs[1]))])
        h.close()
        ctx.close()
        if status[0] != 0:
            print("spp prove: inputs do not satisfy the circuit", file=sys.stderr)
            return 1
        open(base + ".proof", "wb").write(proofs[0])
        open(base + ".pw", "wb").write(pws[0])
        return 0
    ok = verify(open(a.vk, "rb").read(), open(a.proof, "rb").read(), open(a.pw, "rb").read())
    print("verification %s" % ("succeeded" if ok else "FAILED"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
