// MerkleOpenAir (AIR id 16): a batch of Merkle openings of ONE Poseidon tree in one table -- verify_merkle_proof_to_cap (plonky2
// v0.2.0 hash/merkle_proofs.rs) for any number of leaves, what a recursive verifier spends most of its rows on.  One BLOCK is 32
// rows and is exactly a PoseidonAir block (air_library.py poseidon_builder: columns 0..47, one round per row, rows 30 / 31 hold the
// output); a path of D levels is D consecutive blocks, one two-to-one compression each, the paths follow each other and the rest of
// the table is idle blocks (ordinary permutations of the zero state).  Nothing in the table is positional: the shape is carried
// by 18 further columns that are constant over a block,
//     BIT        this level's index bit             SIB[4]   the sibling digest
//     CUR[4]     the node entering this level       LEAF[4]  the leaf digest of the path, carried along
//     R          the index bits not yet consumed (this level's included), LVL the 1-based level
//     ACT        the block belongs to a path        END / FIRSTB   top / first level of its path
// so paths of any depth and any number of them fit this one AIR id at any log_n >= 5.  The structure is cyclic like the running
// sum: every constraint holds on every row, the wrap-around pair included; there are no first-row or last-row constraints.
// Public inputs (9): the root (the Poseidon two-to-one fold of the tree's cap down to one digest; the cap itself at cap height
// 0), the depth D = log2(n_leaves) -- every path has D levels -- and the CLAIMS DIGEST, hash_n_to_hash_no_pad of the list
// (index, d0, d1, d2, d3) of all openings in order.  The table does not constrain the digest: it is a public input so that the
// lookup challenges, which are drawn after the public inputs are observed, depend on the claims -- without it a prover could
// choose the claims after seeing beta.
// Bus: every path sends its opening (R of its first block = the leaf index, LEAF) as the two TAG_OPEN messages of air_bus.cuh;
// the table publishes total / rows.  Whoever holds the openings (vx_merkle_openings_verify; later the leaf-sponge and FRI
// tables of an aggregation proof) receives them: the bus closes iff the proven openings are the claimed ones.
// Constraint ORDER is protocol: tests/merkle_open_ref.py restates it independently.
//
// MerkleOpenSetAir (AIR id 19) is the same table for paths into SEVERAL trees: six more block-constant columns
//     TREE     the tree of the path, carried along it        ROOT[4], DEPTH   the root the path must end in and its number of levels
// replace the root and the depth among the public inputs (4 are left: the digest the table does not constrain).  At END the output
// must be ROOT and LVL must be DEPTH -- WHICH root and depth belong to a tree the table does not know: the END block sends them as
// the two TAG_ROOT messages (TREE, ROOT, DEPTH), and whoever knows the trees (the verifier of vx_fri_queries_verify) receives them.
// The openings go out as open_of(TREE, ...).  Two helpers, one running sum: 6 auxiliary columns.  Both AIRs are one statement of
// the constraints (mop::eval<SET>); tests/fri_queries_ref.py restates the set's order.
#pragma once
#include <vector>

#include "air.cuh"
#include "poseidon_constants.h"

namespace mop {
constexpr int BIT = 48, SIB = 49, CUR = 53, LEAF = 57, R = 61, LVL = 62, ACT = 63, END = 64, FIRSTB = 65, COLS = 66, AUX = 4, PUB = 9;
constexpr int TREE = 66, ROOT = 67, DEPTH = 71, SET_COLS = 72, SET_AUX = 6, SET_PUB = 4;  // MerkleOpenSetAir
constexpr int P_FULL = 12, P_ROUND = 13, P_OUT = 14, P_SPARE = 15, P_FIRST = 16, PERIODIC = 17;  // periodic 0..11: the round constants

inline void periodic_values(std::vector<uint64_t>& v) {
    static const uint64_t RC[360] = VX_POSEIDON_RC_INIT;
    v.assign((size_t)PERIODIC * 32, 0);
    for (int r = 0; r < 30; ++r) {
        for (int i = 0; i < 12; ++i) v[32 * i + r] = RC[12 * r + i];
        v[32 * P_FULL + r] = r < 4 || r >= 26;
        v[32 * P_ROUND + r] = 1;
    }
    v[32 * P_OUT + 30] = 1, v[32 * P_SPARE + 31] = 1, v[32 * P_FIRST + 0] = 1;
}


// the messages of both AIRs (air.cuh): the first block of a path sends its opening; the set's END block the root it ended in as well
template <bool SET, class F, class Row, class Sink>
VX_HD void messages(const Row& loc, const F*, const bus::Bus<X2<F>>& bus, Sink& s) {
    const F r = loc[R];
    if constexpr (SET) {
        const F tree = loc[TREE], depth = loc[DEPTH];
        s.pair(loc[FIRSTB], bus.open_of(tree, r, loc[LEAF], loc[LEAF + 1], bus::K<0>{}), bus.open_of(tree, r, loc[LEAF + 2], loc[LEAF + 3], bus::K<1>{}));
        s.pair(loc[END], bus.root(tree, loc[ROOT], loc[ROOT + 1], bus::K<0>{}, depth), bus.root(tree, loc[ROOT + 2], loc[ROOT + 3], bus::K<1>{}, depth));
    } else {
        s.pair(loc[FIRSTB], bus.open(r, loc[LEAF], loc[LEAF + 1], bus::K<0>{}), bus.open(r, loc[LEAF + 2], loc[LEAF + 3], bus::K<1>{}));
    }
}

// the constraints of both AIRs: Air::SET = false is MerkleOpenAir, true MerkleOpenSetAir
template <class Air, class F, class Row, class Cn>
VX_HD void eval(const Row& loc, const Row& nxt, const F* per, const F* pub, const F* chal, const F* apub, Cn& c) {
    constexpr bool SET = Air::SET;
    constexpr int NC = Air::COLS;
    const F one = F::from(1), full = per[P_FULL], round = per[P_ROUND], out = per[P_OUT], spare = per[P_SPARE], first = per[P_FIRST];
    // ---- 1. the permutation (PoseidonAir): x = s + round constant, a = x^2, b = a^2, t = x a b; y = t in full rounds and for
    // word 0, x otherwise; next s = MDS y on the round rows, next s = s on the output row
    F y[12];  // (the loops that index y / per are unrolled: the arrays stay in registers on the device)
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const F x = loc[i] + per[i];
        c.constraint(loc[12 + i] - x * x);
    }
#pragma unroll 1
    for (int i = 0; i < 12; ++i) c.constraint(loc[24 + i] - loc[12 + i] * loc[12 + i]);
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const F x = loc[i] + per[i], t = loc[36 + i];
        c.constraint(t - x * loc[12 + i] * loc[24 + i]);
        y[i] = i == 0 ? t : full * t + (one - full) * x;
    }
    {
        const uint64_t circ[12] = VX_POSEIDON_MDS_CIRC_INIT;
#pragma unroll
        for (int q = 0; q < 12; ++q) {
            F acc = y[q] * F::from(circ[0] + (q == 0 ? VX_POSEIDON_MDS_DIAG0 : 0));
#pragma unroll
            for (int i = 1; i < 12; ++i) acc = acc + y[(i + q) % 12] * F::from(circ[i]);
            c.constraint(round * (nxt[q] - acc));
        }
    }
#pragma unroll 1
    for (int i = 0; i < 12; ++i) c.constraint(out * (nxt[i] - loc[i]));
    // ---- 2. the 18 (24) shape columns are constant over a block
#pragma unroll 1
    for (int j = BIT; j < NC; ++j) c.constraint((one - spare) * (nxt[j] - loc[j]));
    // ---- 3. flags
    const F bit = loc[BIT], act = loc[ACT], end = loc[END], r = loc[R], lvl = loc[LVL], cont = act - end;
    c.constraint(bit * (bit - one));
    c.constraint(act * (act - one));
    c.constraint(end * (end - one));
    c.constraint(end * (one - act));
    // ---- 4. block input, on the first row: (CUR, SIB) ordered by the index bit, zero capacity
#pragma unroll 1
    for (int i = 0; i < 4; ++i) c.constraint(first * (loc[i] - loc[CUR + i] - bit * (loc[SIB + i] - loc[CUR + i])));
#pragma unroll 1
    for (int i = 0; i < 4; ++i) c.constraint(first * (loc[4 + i] - loc[SIB + i] + bit * (loc[SIB + i] - loc[CUR + i])));
#pragma unroll 1
    for (int i = 8; i < 12; ++i) c.constraint(first * loc[i]);
    // ---- 5. on the spare row (it holds the permutation's output), towards the next block
    {
        const F sc = spare * cont, sn = spare * (one - cont);
#pragma unroll 1
        for (int i = 0; i < 4; ++i) c.constraint(sc * (nxt[CUR + i] - loc[i]));
#pragma unroll 1
        for (int i = 0; i < 4; ++i) c.constraint(sc * (nxt[LEAF + i] - loc[LEAF + i]));
        c.constraint(sc * (r - nxt[R] - nxt[R] - bit));
        c.constraint(sc * (nxt[LVL] - lvl - one));
        c.constraint(sc * (one - nxt[ACT]));
        if constexpr (SET) c.constraint(sc * (nxt[TREE] - loc[TREE]));
#pragma unroll 1
        for (int i = 0; i < 4; ++i) c.constraint(sn * (nxt[CUR + i] - nxt[LEAF + i]));
        c.constraint(sn * (nxt[LVL] - one));
        c.constraint(spare * (nxt[FIRSTB] - nxt[ACT] * (one - cont)));
    }
    // ---- 6. the top of a path: no index bit is left, the level is the tree's depth, the output is the root
    c.constraint(end * (r - bit));
    if constexpr (SET) {
        c.constraint(end * (lvl - loc[DEPTH]));
#pragma unroll 1
        for (int i = 0; i < 4; ++i) c.constraint(spare * end * (loc[i] - loc[ROOT + i]));
    } else {
        c.constraint(end * (lvl - pub[4]));
#pragma unroll 1
        for (int i = 0; i < 4; ++i) c.constraint(spare * end * (loc[i] - pub[i]));
    }
    // ---- 7. the bus (messages above): one helper per message pair, the running sum advances once per block
    bus_constraints<Air>(loc, nxt, per, pub, chal, apub, c);
}
}  // namespace mop

struct MerkleOpenAir {
    static constexpr int ID = 16, COLS = mop::COLS, PUB = mop::PUB, PERIODIC = mop::PERIODIC, PERIOD_LOG = 5, QUOT_ROWS_PER_LANE = 1, AUX = mop::AUX, CHAL = 4, AUXPUB = 1, EXACT_LOG = 0;
    static constexpr int plog(int) { return 5; }
    static int32_t gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub);
    static void periodic_values(std::vector<uint64_t>& v) { mop::periodic_values(v); }
    template <class F, class Row, class Cn>
    __host__ __device__ static void eval(const Row& loc, const Row& nxt, const F* per, const F* pub, const F* chal, const F* apub, Cn& c) {
        mop::eval<MerkleOpenAir>(loc, nxt, per, pub, chal, apub, c);
    }
    static constexpr bool SET = false;
    static constexpr int N_HELP = 1, BUS_ROWS = 32, BUS_STEP = mop::P_FIRST, BUS_BLOCK = 64, BUS_PERIODIC = 0;
    template <class F, class Row, class Sink>
    VX_HD static void messages(const Row& loc, const F*, const F* pub, const bus::Bus<X2<F>>& bus, Sink& s) {
        mop::messages<SET>(loc, pub, bus, s);
    }
};

struct MerkleOpenSetAir {
    static constexpr int ID = 19, COLS = mop::SET_COLS, PUB = mop::SET_PUB, PERIODIC = mop::PERIODIC, PERIOD_LOG = 5, QUOT_ROWS_PER_LANE = 1, AUX = mop::SET_AUX, CHAL = 4, AUXPUB = 1, EXACT_LOG = 0;
    static constexpr int plog(int) { return 5; }
    static int32_t gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub);
    static void periodic_values(std::vector<uint64_t>& v) { mop::periodic_values(v); }
    template <class F, class Row, class Cn>
    __host__ __device__ static void eval(const Row& loc, const Row& nxt, const F* per, const F* pub, const F* chal, const F* apub, Cn& c) {
        mop::eval<MerkleOpenSetAir>(loc, nxt, per, pub, chal, apub, c);
    }
    static constexpr bool SET = true;
    static constexpr int N_HELP = 2, BUS_ROWS = 32, BUS_STEP = mop::P_FIRST, BUS_BLOCK = 64, BUS_PERIODIC = 0;
    template <class F, class Row, class Sink>
    VX_HD static void messages(const Row& loc, const F*, const F* pub, const bus::Bus<X2<F>>& bus, Sink& s) {
        mop::messages<SET>(loc, pub, bus, s);
    }
};
