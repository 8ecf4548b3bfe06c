"""TEST INFRASTRUCTURE: ARBITRARY data for the quotient evaluation of every compiled AIR (vx_quotient_eval_aux) and the independent
restatement each one is compared with -- shared by test_gpu_quotient_arbitrary.py (the GPU comparison), test_quotient_mutants.py
(the CPU measurement of what such data can tell apart) and test_oracle_stark.py.  No tests here.

The data is neither a trace nor an LDE of one: on a satisfying trace many cells are tied to each other (block-constant columns,
flags that are prefixes of one another, copies), and a compiled constraint that reads the wrong one of two tied cells gives the
same quotient.  Uniform words with a third from the edge list of the fused multiply (air_program_fuzz.special_words) tie nothing.

An AIR is named by the expression that gives its id in the binding, "VX_AIR_SHA_TREE[16]" for lib.VX_AIR_SHA_TREE[16]."""
import re

import numpy as np

import air_program_fuzz as Z

P = Z.P


def restatements():
    """AIR name -> a function that returns its restatement (imported on demand: the bus tables assemble programs)."""
    from oracle import blake_air, ed_air, epoch_air, sha512_air, sha_air, sha_tree_air
    from oracle import stark_ref as S
    import fri_combine_ref
    import fri_fold_ref
    import fri_queries_ref
    import leaf_noop_ref
    import leaf_sponge_ref
    import merkle_open_ref
    import transcript_ref

    return {
        "VX_AIR_FIBONACCI": lambda: S.FibAir, "VX_AIR_MIX": lambda: S.MixAir, "VX_AIR_LOOKUP": lambda: S.LookupAir,
        "VX_AIR_SHA_CHAIN": lambda: sha_air.ShaChainAir, "VX_AIR_BLAKE_CHAIN": lambda: blake_air.BlakeChainAir,
        "VX_AIR_SHA_TREE[16]": lambda: sha_tree_air.make_air(16), "VX_AIR_ED25519[16]": lambda: ed_air.make_air(16),
        "VX_AIR_SHA512[10]": lambda: sha512_air.make_air(10), "VX_AIR_EPOCH_END": lambda: epoch_air.EpochEndAir,
        "VX_AIR_MERKLE_OPEN": merkle_open_ref.air, "VX_AIR_LEAF_SPONGE": leaf_sponge_ref.air, "VX_AIR_FRI_FOLD": fri_fold_ref.air,
        "VX_AIR_MERKLE_OPEN_SET": fri_queries_ref.open_air, "VX_AIR_LEAF_SPONGE_SET": fri_queries_ref.sponge_air,
        "VX_AIR_FRI_COMBINE": fri_combine_ref.air, "VX_AIR_LEAF_NOOP": leaf_noop_ref.air, "VX_AIR_TRANSCRIPT": transcript_ref.air,
    }


# the eight tables of the buses, whose restatements are constraint programs
BUS_TABLES = ["VX_AIR_MERKLE_OPEN", "VX_AIR_LEAF_SPONGE", "VX_AIR_FRI_FOLD", "VX_AIR_MERKLE_OPEN_SET", "VX_AIR_LEAF_SPONGE_SET", "VX_AIR_FRI_COMBINE",
              "VX_AIR_LEAF_NOOP", "VX_AIR_TRANSCRIPT"]
_made = {}


def restatement(name):
    if name not in _made:
        _made[name] = restatements()[name]()
    return _made[name]


AIR_NAME = re.compile(r"VX_AIR_[A-Z0-9_]+(?:\[\d+\])?")


def air_id(lib, name):
    """the id the binding `lib` gives the AIR `name`"""
    m = re.fullmatch(r"(VX_AIR_[A-Z0-9_]+)(?:\[(\d+)\])?", name)
    v = getattr(lib, m.group(1))
    return v[int(m.group(2))] if m.group(2) else v


def binding_air_ids(lib):
    """name -> id of every compiled AIR the binding names (VX_AIR_* integers and the entries of the VX_AIR_* tables)"""
    out = {}
    for k in dir(lib):
        v = getattr(lib, k)
        if k.startswith("VX_AIR_") and k != "VX_AIR_USER_BASE":
            if isinstance(v, dict):
                out.update({"%s[%d]" % (k, kk): vv for kk, vv in v.items()})
            elif isinstance(v, int):
                out[k] = v
    return out


def words(rng, n):
    """n random canonical words as Python integers"""
    return [int(v) for v in rng.integers(0, P, size=n, dtype=np.uint64)]


def n_columns(air):
    return air.COLS + getattr(air, "AUX", 0)


def seed_of(name, log_n, rate_bits):
    return [sum(name.encode()), log_n, rate_bits]


def statement_words(rng, air):
    """-> (public inputs, lookup challenges, published auxiliary words): random canonical"""
    return words(rng, air.PUB), words(rng, getattr(air, "CHAL", 0)), words(rng, 2 * getattr(air, "AUXPUB", 0))


def alpha_pairs(rng):
    """the three constraint-challenge pairs every case is evaluated under: a random pair, (1, p - 1) (every power is +-1), and
    (0, r), which leaves only the last constraint in the first accumulator"""
    return [("random", words(rng, 2)), ("(1, p-1)", [1, P - 1]), ("(0, r)", [0] + words(rng, 1))]


def arbitrary(name, log_n, rate_bits):
    """-> (air, lde [COLS + AUX][N], public inputs, challenges, published words, alpha pairs) of one host-filled case"""
    air = restatement(name)
    rng = np.random.default_rng(seed_of(name, log_n, rate_bits))
    lde = Z.special_lde(rng, n_columns(air), 1 << (log_n + rate_bits))
    pub, chal, apub = statement_words(rng, air)
    return air, lde, pub, chal, apub, alpha_pairs(rng)


def sample_points(rng, log_N, k):
    """0, N - 1, every 2^b - 1 and N - 2^b (runs of ones at the bottom and at the top of the index: each limb of the three-level
    root table at its largest), runs of ones in the middle, and k random indices."""
    N = 1 << log_N
    pts = {0, N - 1}
    for b in range(1, log_N + 1):
        pts.add((1 << b) - 1)
        pts.add(N - (1 << (b - 1)))
    for lo, hi in ((11, 22), (22, 32), (0, 11)):
        lo, hi = min(lo, log_N), min(hi, log_N)
        pts.add(((1 << hi) - 1) ^ ((1 << lo) - 1))
    pts.update(int(v) for v in rng.integers(0, N, size=k))
    return sorted(p for p in pts if 0 <= p < N)


def reference(air, lde, pub, chal, apub, alphas, log_n, rate_bits, points=None, nxt_rows=None):
    from oracle import stark_ref as S

    aux = getattr(air, "AUX", 0)
    return S.quotient_values(air, lde, pub, alphas, log_n, rate_bits, chal if aux else None, apub if aux else None, points=points, nxt_rows=nxt_rows)
