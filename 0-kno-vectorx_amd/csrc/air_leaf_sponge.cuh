// LeafSpongeAir (AIR id 17): the opened leaf ROWS of one Poseidon tree hashed in one table -- hash_n_to_hash_no_pad (plonky2 v0.2.0
// hash/hashing.rs hash_n_to_m_no_pad) for any number of leaves of one length L >= 5, the second table of proof aggregation.  It
// sits on one logUp bus with MerkleOpenAir (air_merkle_open.cuh): that table proves that a leaf DIGEST lies in the tree, this one
// that the digest is the hash of the row the verifier holds.  One BLOCK is 32 rows and is exactly a PoseidonAir block (columns
// 0..47, one round per row, rows 30 / 31 hold the output); a leaf is B = ceil(L / 8) consecutive blocks, block k absorbs the
// words 8k .. 8k + 7 by OVERWRITING the rate part of the state and carries the capacity (zero in the first block); the last
// block of a leaf with t = L mod 8 != 0 overwrites its first t rate words only, the others keep the previous output (zero when
// there is none: L < 8).  The digest is the first four words of the last block's output.  The leaves follow each other and the
// rest of the table is idle blocks (permutations of the zero state).  Nothing in the table is positional: the shape is carried by
// 18 further columns that are constant over a block,
//     MSG[8]   the rate part entering the permutation: the absorbed words, and behind a tail the words that are kept
//     IDX      the leaf index, carried over the blocks of a leaf        POS   the block number within the leaf
//     ACT      the block belongs to a leaf       FIRSTB / LASTB   first / last block of its leaf
//     NXL      the NEXT block continues this leaf and is its last one (a helper flag: it keeps the tail rule at degree 3)
//     DIG[4]   the first four words of this block's output (the bus messages are built from block-constant columns)
// so leaves of any length and any number of them fit this one AIR id at any log_n >= 5.  Every constraint holds on every row
// pair, the wrap-around included; there are no first-row or last-row constraints.
// Public inputs (14): L, B, the eight tail flags w_i = [i < (t or 8)] -- word i of a LAST block is absorbed -- and the ROW-CLAIMS
// DIGEST, hash_n_to_hash_no_pad of the list (index, row[0 .. L)) of all openings in order.  The table does not constrain the
// digest: it is a public input so that the lookup challenges depend on the claims (as in MerkleOpenAir).
// Bus: every active block SENDS its absorbed words as TAG_ROW messages (IDX, 8 POS + i, MSG[i]) -- multiplicity ACT - LASTB (1 -
// w_i): the words a tail keeps are not sent -- and the last block of a leaf RECEIVES the two TAG_OPEN messages (IDX, DIG) that
// MerkleOpenAir sends.  Ten messages, two per extension helper; one cyclic running sum; the table publishes total / rows.
// Constraint ORDER is protocol: tests/leaf_sponge_ref.py restates it independently.
//
// LeafSpongeSetAir (AIR id 20) is the same table for rows of SEVERAL trees of one leaf length: one more block-constant column
// TREE, carried within a leaf; the words go out as row_of(TREE, ...) and the digest is received as open_of(TREE, ...), what
// MerkleOpenSetAir sends.  L, B and the tail flags stay public inputs, so all trees of one table share a leaf length (a per-tree
// length would need the tail flags as cells, and the tail rule is at degree 3 already); because the messages name their tree,
// several such tables of different lengths can share a bus.  Both AIRs are one statement of the constraints (lsp::eval<SET>);
// tests/fri_queries_ref.py restates the set's order.
#pragma once
#include <vector>

#include "air.cuh"
#include "poseidon_constants.h"

namespace lsp {
constexpr int MSG = 48, IDX = 56, POS = 57, ACT = 58, FIRSTB = 59, LASTB = 60, NXL = 61, DIG = 62, COLS = 66, N_HELP = 5, AUX = 2 * N_HELP + 2;
constexpr int TREE = 66, SET_COLS = 67;  // LeafSpongeSetAir
constexpr int PUB_L = 0, PUB_B = 1, PUB_W = 2, PUB_DIGEST = 10, PUB = 14;
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


// the messages of both AIRs (air.cuh): eight row words sent, the two halves of the digest received; the set's messages name their tree
template <bool SET, class F, class Row, class Sink>
VX_HD void messages(const Row& loc, const F* pub, const bus::Bus<X2<F>>& bus, Sink& s) {
    const F idx = loc[IDX], last = loc[LASTB], cont = loc[ACT] - last, pos8 = loc[POS] * F::from(8);
    auto d_row = [&](const F& position, const F& word) {
        if constexpr (SET) return bus.row_of(loc[TREE], idx, position, word);
        else return bus.row(idx, position, word);
    };
    auto d_open = [&](const F& da, const F& db, auto half) {
        if constexpr (SET) return bus.open_of(loc[TREE], idx, da, db, half);
        else return bus.open(idx, da, db, half);
    };
#pragma unroll Sink::UNROLL
    for (int e = 0; e < 4; ++e) {  // multiplicity ACT - LASTB (1 - w_i): the words a tail keeps are not sent
        const F ma = cont + last * pub[PUB_W + 2 * e], mb = cont + last * pub[PUB_W + 2 * e + 1];
        const F pa = pos8 + F::from((uint64_t)(2 * e)), pb = pos8 + F::from((uint64_t)(2 * e + 1));
        s.put(ma, d_row(pa, loc[MSG + 2 * e]), mb, d_row(pb, loc[MSG + 2 * e + 1]));
    }
    s.pair(F::from(0) - last, d_open(loc[DIG], loc[DIG + 1], bus::K<0>{}), d_open(loc[DIG + 2], loc[DIG + 3], bus::K<1>{}));
}

// the constraints of both AIRs: Air::SET = false is LeafSpongeAir, true LeafSpongeSetAir
template <class Air, class F, class Row, class Cn>
VX_HD void eval(const Row& loc, const Row& nxt, const F* per, const F* pub, const F* chal, const F* apub, Cn& c) {
    constexpr bool SET = Air::SET;
    constexpr int NC = Air::COLS;
    const F one = F::from(1), full = per[P_FULL], round = per[P_ROUND], out = per[P_OUT], spare = per[P_SPARE], first = per[P_FIRST];
    // ---- 1. the permutation (PoseidonAir, as in MerkleOpenAir): x = s + round constant, a = x^2, b = a^2, t = x a b; y = t in
    // full rounds and for word 0, x otherwise; next s = MDS y on the round rows, next s = s on the output row
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
    // ---- 2. the 18 (19) shape columns are constant over a block
#pragma unroll 1
    for (int j = MSG; j < NC; ++j) c.constraint((one - spare) * (nxt[j] - loc[j]));
    // ---- 3. flags
    const F idx = loc[IDX], pos = loc[POS], act = loc[ACT], firstb = loc[FIRSTB], last = loc[LASTB], nxl = loc[NXL], cont = act - last;
    c.constraint(act * (act - one));
    c.constraint(last * (last - one));
    c.constraint(last * (one - act));
    // ---- 4. block input, on the first row: the rate part is MSG
#pragma unroll 1
    for (int i = 0; i < 8; ++i) c.constraint(first * (loc[i] - loc[MSG + i]));
    // ---- 5. on the spare row (it holds the permutation's output), towards the next block
    {
        const F sc = spare * cont, sn = spare * (one - cont);
#pragma unroll 1
        for (int i = 8; i < 12; ++i) c.constraint(sc * (nxt[i] - loc[i]));  // the capacity is carried within a leaf
#pragma unroll 1
        for (int i = 8; i < 12; ++i) c.constraint(sn * nxt[i]);  // ... and zero where a leaf (or an idle block) starts
        c.constraint(sc * (nxt[IDX] - idx));
        c.constraint(sc * (nxt[POS] - pos - one));
        c.constraint(sc * (one - nxt[ACT]));
        if constexpr (SET) c.constraint(sc * (nxt[TREE] - loc[TREE]));
        c.constraint(spare * (nxt[FIRSTB] - nxt[ACT] * (one - cont)));
        c.constraint(spare * (nxl - cont * nxt[LASTB]));
#pragma unroll 1
        for (int i = 0; i < 4; ++i) c.constraint(spare * (loc[DIG + i] - loc[i]));
        // the tail rule: a word the last block does not absorb keeps the previous output
        const F sl = spare * nxl;
#pragma unroll 1
        for (int i = 0; i < 8; ++i) c.constraint(sl * ((nxt[MSG + i] - loc[i]) * (one - pub[PUB_W + i])));
    }
    // ---- 6. every leaf has exactly B blocks; a single-block leaf (L < 8) keeps zero behind its tail
    c.constraint(firstb * pos);
    c.constraint(last * (pos + one - pub[PUB_B]));
    {
        const F fl = firstb * last;
#pragma unroll 1
        for (int i = 0; i < 8; ++i) c.constraint(fl * (loc[MSG + i] * (one - pub[PUB_W + i])));
    }
    // ---- 7. the bus (messages above): two messages per helper, the running sum advances once per block
    bus_constraints<Air>(loc, nxt, per, pub, chal, apub, c);
}
}  // namespace lsp

struct LeafSpongeAir {
    static constexpr int ID = 17, COLS = lsp::COLS, PUB = lsp::PUB, PERIODIC = lsp::PERIODIC, PERIOD_LOG = 5, QUOT_ROWS_PER_LANE = 1, AUX = lsp::AUX, CHAL = 4, AUXPUB = 1, EXACT_LOG = 0;
    static constexpr int plog(int) { return 5; }
    static int32_t gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub);
    static void periodic_values(std::vector<uint64_t>& v) { lsp::periodic_values(v); }
    template <class F, class Row, class Cn>
    __host__ __device__ static void eval(const Row& loc, const Row& nxt, const F* per, const F* pub, const F* chal, const F* apub, Cn& c) {
        lsp::eval<LeafSpongeAir>(loc, nxt, per, pub, chal, apub, c);
    }
    static constexpr bool SET = false;
    static constexpr int N_HELP = lsp::N_HELP, BUS_ROWS = 32, BUS_STEP = lsp::P_FIRST, BUS_BLOCK = 64, BUS_PERIODIC = 0;
    template <class F, class Row, class Sink>
    VX_HD static void messages(const Row& loc, const F*, const F* pub, const bus::Bus<X2<F>>& bus, Sink& s) {
        lsp::messages<SET>(loc, pub, bus, s);
    }
};

struct LeafSpongeSetAir {
    static constexpr int ID = 20, COLS = lsp::SET_COLS, PUB = lsp::PUB, PERIODIC = lsp::PERIODIC, PERIOD_LOG = 5, QUOT_ROWS_PER_LANE = 1, AUX = lsp::AUX, CHAL = 4, AUXPUB = 1, EXACT_LOG = 0;
    static constexpr int plog(int) { return 5; }
    static int32_t gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub);
    static void periodic_values(std::vector<uint64_t>& v) { lsp::periodic_values(v); }
    template <class F, class Row, class Cn>
    __host__ __device__ static void eval(const Row& loc, const Row& nxt, const F* per, const F* pub, const F* chal, const F* apub, Cn& c) {
        lsp::eval<LeafSpongeSetAir>(loc, nxt, per, pub, chal, apub, c);
    }
    static constexpr bool SET = true;
    static constexpr int N_HELP = lsp::N_HELP, BUS_ROWS = 32, BUS_STEP = lsp::P_FIRST, BUS_BLOCK = 64, BUS_PERIODIC = 0;
    template <class F, class Row, class Sink>
    VX_HD static void messages(const Row& loc, const F*, const F* pub, const bus::Bus<X2<F>>& bus, Sink& s) {
        lsp::messages<SET>(loc, pub, bus, s);
    }
};
