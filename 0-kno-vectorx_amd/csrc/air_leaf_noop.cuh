// LeafNoopAir (AIR id 22): the openings of NO-OP leaves -- a Poseidon tree whose leaves have at most 4 words does not hash them
// (plonky2 v0.2.0 hash/hash_types.rs hash_or_noop): the leaf digest IS the row, zero-padded to 4 words.  That is the quotient
// tree of every vx_stark_prove proof and any other commitment tree of at most 4 columns.  For such a tree MerkleOpenSetAir sends
// the digest as two open_of(tree, index, ., ., half) messages while FriCombineAir receives the row one word per message,
// row_of(tree, index, position, word); this table is the adapter between the two, the no-op counterpart of LeafSpongeSetAir.
// One ROW per opening, 11 columns:
//     ACT      the row is an opening        TREE, IDX   its tree and leaf index
//     W[4]     the row's words, zero behind its length
//     E[4]     E_j = word j exists: E_0 = ACT, the flags only fall (no gap), and a word that does not exist is zero
// The length of a leaf is E_0 + .. + E_3 and is NOT a public input: one table carries leaves of different lengths (the main tree
// of FibAir at 2 and the quotient tree at 4 in the tests).  What forces the flags is the balance of the bus: the receiver's public
// cm / ca / nq say which (tree, index, position) words must arrive, a word sent beyond them or missing below them leaves a term
// nobody cancels, and a word claimed not to exist must be the zero the digest holds there.
// Idle rows are all zero.  Nothing is positional: every constraint holds on every row pair, the wrap-around included; there are
// no first-row or last-row constraints and no periodic columns, so any number of openings fits this one AIR id at any log_n >= 5.
// Public inputs (4): a digest the table does not constrain (it makes the lookup challenges depend on the claims, as in
// MerkleOpenSetAir / LeafSpongeSetAir).
// Bus: an active row RECEIVES open_of(TREE, IDX, W0, W1, 0) and open_of(TREE, IDX, W2, W3, 1) -- what MerkleOpenSetAir sends --
// and SENDS row_of(TREE, IDX, j, W_j) with multiplicity E_j.  Six messages, two per extension helper; one cyclic running sum; the
// table publishes total / rows.  No new bus tag.
// Constraint ORDER is protocol: tests/leaf_noop_ref.py restates it independently.
#pragma once
#include <vector>

#include "air.cuh"

namespace lnp {
constexpr int ACT = 0, TREE = 1, IDX = 2, W = 3, E = 7, COLS = 11, N_HELP = 3, AUX = 2 * N_HELP + 2;
constexpr int PUB_DIGEST = 0, PUB = 4;
constexpr int MAX_LEN = 4;  // hash_or_noop: a leaf of at most 4 words is its own digest
}  // namespace lnp

struct LeafNoopAir {
    static constexpr int ID = 22, COLS = lnp::COLS, PUB = lnp::PUB, PERIODIC = 0, PERIOD_LOG = 0, QUOT_ROWS_PER_LANE = 1, AUX = lnp::AUX, CHAL = 4, AUXPUB = 1, EXACT_LOG = 0;
    static constexpr int plog(int) { return 0; }
    static int32_t gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub);
    static void periodic_values(std::vector<uint64_t>& v) { v.clear(); }

    static constexpr int N_HELP = lnp::N_HELP, BUS_ROWS = 1, BUS_STEP = -1, BUS_BLOCK = 256, BUS_PERIODIC = 0;

    // the two halves of the digest received, the words that exist sent
    template <class F, class Row, class Sink>
    VX_HD static void messages(const Row& loc, const F*, const F*, const bus::Bus<X2<F>>& bus, Sink& s) {
        using namespace lnp;
        const F tree = loc[TREE], idx = loc[IDX];
        s.pair(F::from(0) - loc[ACT], bus.open_of(tree, idx, loc[W], loc[W + 1], bus::K<0>{}), bus.open_of(tree, idx, loc[W + 2], loc[W + 3], bus::K<1>{}));
#pragma unroll
        for (int e = 0; e < 2; ++e)
            s.put(loc[E + 2 * e], bus.row_of(tree, idx, F::from((uint64_t)(2 * e)), loc[W + 2 * e]), loc[E + 2 * e + 1], bus.row_of(tree, idx, F::from((uint64_t)(2 * e + 1)), loc[W + 2 * e + 1]));
    }

    template <class F, class Row, class Cn>
    __host__ __device__ static void eval(const Row& loc, const Row& nxt, const F*, const F*, const F* chal, const F* apub, Cn& c) {
        using namespace lnp;
        const F one = F::from(1), act = loc[ACT];
        // ---- 1. boolean cells
        c.constraint(act * (act - one));
#pragma unroll
        for (int j = 0; j < 4; ++j) c.constraint(loc[E + j] * (loc[E + j] - one));
        // ---- 2. the length: word 0 exists exactly on an opening, the flags only fall, a word that does not exist is zero
        c.constraint(loc[E] - act);
#pragma unroll
        for (int j = 0; j < 3; ++j) c.constraint(loc[E + j + 1] * (one - loc[E + j]));
#pragma unroll
        for (int j = 0; j < 4; ++j) c.constraint((one - loc[E + j]) * loc[W + j]);
        // ---- 3. the bus (messages below)
        bus_constraints<LeafNoopAir>(loc, nxt, (const F*)nullptr, (const F*)nullptr, chal, apub, c);
    }
};
