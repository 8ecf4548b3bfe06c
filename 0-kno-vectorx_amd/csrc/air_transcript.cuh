// TranscriptAir (AIR id 23): the Fiat-Shamir transcripts of 1..64 inner proofs -- CHAINS -- in one table: the duplex challenger of
// plonky2 v0.2.0 iop/challenger.rs (glh::Challenger: width 12, rate 8, overwrite mode), absorbing and squeezing interleaved.  One
// BLOCK is 32 rows and is exactly a PoseidonAir block (columns 0..47, one round per row, rows 30 / 31 hold the output), as in
// LeafSpongeAir; a block is ONE duplex of a chain: it overwrites the first k rate words of the state with absorbed words, permutes,
// and q challenges are popped from the END of its output (the challenger returns out[--n_out]).  The chains follow each other and
// the rest of the table is idle blocks (permutations of the zero state).  Nothing is positional: the shape is carried by 45 further
// columns that are constant over a block,
//     MSG[8]   the rate part entering the permutation           W[8]   word i is absorbed in this block: a prefix
//     OUT[8]   the rate part of the output                      Q[8]   out[i] is drawn as a challenge: a suffix
//     PREV[8]  the rate part the previous block of the chain left (zero in a START block and in an idle one)
//     CHAIN    the chain id        ACT   the block belongs to a chain        START   it is the first block of its chain
//     NABS / NCH   words absorbed / challenges drawn by the chain BEFORE this block
// so any number of chains of any length fits this one AIR id at any log_n >= 5.  Every constraint holds on every row pair, the
// wrap-around included; there are no first-row or last-row constraints.
// State: a word that is not absorbed keeps the previous output (MSG_i = PREV_i), the capacity is carried within a chain; a START
// block enters from the zero state with NABS = NCH = 0 and zero behind its absorbed prefix; idle blocks have W = Q = 0.
// The plan of a chain is forced by three rules (with the bus below): an active block absorbs or squeezes, ACT (1 - W_0)(1 - Q_7) = 0;
// a block that absorbs fewer than 8 words squeezes, ACT (1 - W_7)(1 - Q_7) = 0 -- the challenger duplexes on a full buffer or on a
// challenge only --; and a block that absorbs nothing follows a block of its chain that was squeezed dry (Q_0 = 1 there) and is
// no START.  "Active and absorbs nothing" is the linear ACT - W_0 (W_0 = 1 only in an active block), "the next block continues this
// chain" the linear ACT' - START': no helper flag is needed to stay at degree 3.
// Public inputs (4): a statement digest the table does not constrain (it makes the lookup challenges depend on the claims, as in
// MerkleOpenSetAir / LeafSpongeSetAir / LeafNoopAir).
// Bus: an active block RECEIVES obs(CHAIN, NABS + i, MSG_i) with multiplicity W_i and SENDS chal(CHAIN, NCH + 7 - i, NABS + sum W,
// OUT_i) with multiplicity Q_i.  Sixteen messages, two per extension helper; one cyclic running sum; the table publishes total / rows.
// Constraint ORDER is protocol: tests/transcript_ref.py restates it independently.
#pragma once
#include <vector>

#include "air.cuh"
#include "air_leaf_sponge.cuh"

namespace tsc {
constexpr int MSG = 48, W = 56, OUT = 64, Q = 72, PREV = 80, CHAIN = 88, ACT = 89, START = 90, NABS = 91, NCH = 92, COLS = 93, N_HELP = 8, AUX = 2 * N_HELP + 2;
constexpr int PUB_DIGEST = 0, PUB = 4;
constexpr int MAX_CHAINS = 64;
using lsp::P_FIRST;
using lsp::P_FULL;
using lsp::P_OUT;
using lsp::P_ROUND;
using lsp::P_SPARE;
using lsp::PERIODIC;  // the periodic columns are LeafSpongeAir's: round constants, full, round, output, spare, first
}  // namespace tsc

struct TranscriptAir {
    static constexpr int ID = 23, COLS = tsc::COLS, PUB = tsc::PUB, PERIODIC = tsc::PERIODIC, PERIOD_LOG = 5, QUOT_ROWS_PER_LANE = 1, AUX = tsc::AUX, CHAL = 4, AUXPUB = 1, EXACT_LOG = 0;
    static constexpr int plog(int) { return 5; }
    static int32_t gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub);
    static void periodic_values(std::vector<uint64_t>& v) { lsp::periodic_values(v); }

    static constexpr int N_HELP = tsc::N_HELP, BUS_ROWS = 32, BUS_STEP = tsc::P_FIRST, BUS_BLOCK = 64, BUS_PERIODIC = 0;

    // eight absorbed words received with multiplicity W_i, eight outputs sent with multiplicity Q_i
    template <class F, class Row, class Sink>
    VX_HD static void messages(const Row& loc, const F*, const F*, const bus::Bus<X2<F>>& bus, Sink& s) {
        using namespace tsc;
        const F zero = F::from(0), chain = loc[CHAIN], nabs = loc[NABS], nch = loc[NCH];
        F sw = loc[W];  // (the sum eval has: one expression, one computation)
#pragma unroll
        for (int i = 1; i < 8; ++i) sw = sw + loc[W + i];
        const F absorbed = nabs + sw;
#pragma unroll Sink::UNROLL
        for (int e = 0; e < 4; ++e)
            s.put(zero - loc[W + 2 * e], bus.obs(chain, nabs + F::from((uint64_t)(2 * e)), loc[MSG + 2 * e]), zero - loc[W + 2 * e + 1],
                  bus.obs(chain, nabs + F::from((uint64_t)(2 * e + 1)), loc[MSG + 2 * e + 1]));
#pragma unroll Sink::UNROLL
        for (int e = 0; e < 4; ++e)
            s.put(loc[Q + 2 * e], bus.chal(chain, nch + F::from((uint64_t)(7 - 2 * e)), absorbed, loc[OUT + 2 * e]), loc[Q + 2 * e + 1],
                  bus.chal(chain, nch + F::from((uint64_t)(6 - 2 * e)), absorbed, loc[OUT + 2 * e + 1]));
    }

    template <class F, class Row, class Cn>
    __host__ __device__ static void eval(const Row& loc, const Row& nxt, const F* per, const F*, const F* chal, const F* apub, Cn& c) {
        using namespace tsc;
        const F one = F::from(1), full = per[P_FULL], round = per[P_ROUND], out = per[P_OUT], spare = per[P_SPARE], first = per[P_FIRST];
        // ---- 1. the permutation (PoseidonAir, as in LeafSpongeAir)
        F y[12];
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
        // ---- 2. the 45 shape columns are constant over a block
#pragma unroll 1
        for (int j = MSG; j < COLS; ++j) c.constraint((one - spare) * (nxt[j] - loc[j]));
        // ---- 3. flags: boolean, W a prefix, Q a suffix, nothing absorbed or drawn outside a chain, a START is active
        const F chain = loc[CHAIN], act = loc[ACT], start = loc[START], nabs = loc[NABS], nch = loc[NCH];
        c.constraint(act * (act - one));
        c.constraint(start * (start - one));
        c.constraint(start * (one - act));
#pragma unroll 1
        for (int i = 0; i < 8; ++i) c.constraint(loc[W + i] * (loc[W + i] - one));
#pragma unroll 1
        for (int i = 0; i < 8; ++i) c.constraint(loc[Q + i] * (loc[Q + i] - one));
#pragma unroll 1
        for (int i = 0; i < 7; ++i) c.constraint(loc[W + i + 1] * (one - loc[W + i]));
#pragma unroll 1
        for (int i = 0; i < 7; ++i) c.constraint(loc[Q + i] * (one - loc[Q + i + 1]));
        c.constraint((one - act) * loc[W]);
        c.constraint((one - act) * loc[Q + 7]);
        // ---- 4. the plan: absorb or squeeze; a partial absorption squeezes; a block that absorbs nothing is no START
        c.constraint(act * (one - loc[W]) * (one - loc[Q + 7]));
        c.constraint(act * (one - loc[W + 7]) * (one - loc[Q + 7]));
        c.constraint((act - loc[W]) * start);
        c.constraint(start * nabs);
        c.constraint(start * nch);
        // ---- 5. block input, on the first row: the rate part is MSG; a word that is not absorbed keeps what the chain's previous
        // block left, zero in a START block and in an idle one
#pragma unroll 1
        for (int i = 0; i < 8; ++i) c.constraint(first * (loc[i] - loc[MSG + i]));
#pragma unroll 1
        for (int i = 0; i < 8; ++i) c.constraint((one - loc[W + i]) * (loc[MSG + i] - (act - start) * loc[PREV + i]));
        // ---- 6. on the spare row (it holds the permutation's output), towards the next block; cn: it continues this chain
        {
            F sw = loc[W], sq = loc[Q];
#pragma unroll
            for (int i = 1; i < 8; ++i) sw = sw + loc[W + i], sq = sq + loc[Q + i];
            const F cn = nxt[ACT] - nxt[START], sc = spare * cn, sn = spare * (one - cn);
#pragma unroll 1
            for (int i = 0; i < 8; ++i) c.constraint(spare * (loc[OUT + i] - loc[i]));
#pragma unroll 1
            for (int i = 0; i < 8; ++i) c.constraint(sc * (nxt[PREV + i] - loc[i]));
#pragma unroll 1
            for (int i = 0; i < 8; ++i) c.constraint(sn * nxt[PREV + i]);
#pragma unroll 1
            for (int i = 8; i < 12; ++i) c.constraint(sc * (nxt[i] - loc[i]));  // the capacity is carried within a chain
#pragma unroll 1
            for (int i = 8; i < 12; ++i) c.constraint(sn * nxt[i]);  // ... and zero where a chain (or an idle block) starts
            c.constraint(sc * (one - act));  // a chain is contiguous
            c.constraint(sc * (nxt[CHAIN] - chain));
            c.constraint(sc * (nxt[NABS] - nabs - sw));
            c.constraint(sc * (nxt[NCH] - nch - sq));
            // a block that absorbs nothing follows one that was squeezed dry
            c.constraint(spare * (nxt[ACT] - nxt[W]) * (one - loc[Q]));
        }
        // ---- 7. the bus (messages above): two messages per helper, the running sum advances once per block
        bus_constraints<TranscriptAir>(loc, nxt, per, (const F*)nullptr, chal, apub, c);
    }
};
