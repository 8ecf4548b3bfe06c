// FriFoldAir (AIR id 18): the FRI fold chain of every query of one inner proof in one table -- the per-query loop of
// verify_fri_proof (plonky2 v0.2.0 fri/verifier.rs fri_verifier_query_round: compute_evaluation, x <- x^arity, index >>= arity
// bits; vx_verify.hip does the same on the host) at arity 16, the third table of proof aggregation.  For an inner proof with an
// LDE of 2^LN points, NL >= 1 fold layers with challenges beta_l and FB = LN - 4 NL >= 1 index bits left behind the last layer, a
// query (index, ev_0) is NL FOLD rows followed by FB BIT rows:
//   fold row l   holds the 16 extension values of the query's leaf in layer l, the digit within_l = (index >> 4l) & 15 as four
//                bits and a 16-cell one-hot, and checks leaf[within_l] = ev_l; it interpolates the coset at beta_l by four
//                arity-2 levels  v' = (u + w) / 2 + beta^(2^j) (u - w) c,  c = 1 / (2 y)  for the pair's point y, and hands
//                ev_(l+1) to the next row.  Points are handled by INVERSES: Y = 1 / x_l, the inverse of the coset base is
//                SI = Y g^bitrev(within) (g the 16th root of unity; the factor is a degree-1 sum over the one-hot), S1..S3 its
//                squares, and the next row's Y is S3^2 = Y^16
//   bit row      consumes one of the remaining index bits
// so that R, "the index bits not yet consumed", goes R = 16 Q + within (fold) / R = 2 Q + bit (bit row), next R = Q, and the
// query's LAST row has Q = 0: no bit is left.  (Without that closing rule a wrong digit could be hidden by continuing R with
// field divisions.)  A row counter CNT runs from 0 to NL + FB - 1 over the query; a fold row may be followed by a non-fold row
// only at CNT + 1 = NL and a non-first fold row only follows a fold row, so the fold rows are exactly the rows CNT < NL.
// 1 / x_0 (Y0, carried over the query) is bound to the index by a square-and-multiply accumulator that every row advances by
// its own bits, A <- A^2 w^(-bit), four times on a fold row and once on a bit row -- MSB-first exponentiation by bitrev(index,
// LN), because a digit's low bit comes first -- and on the last row Y0 = 7^-1 A_final: x_0 = 7 w^bitrev(index).
// The queries follow each other and idle rows (all zero) fill the rest.  Nothing is positional: every constraint holds on every
// row pair, the wrap-around included, there are no first-row or last-row constraints and no periodic columns, so any number of
// queries of any shape (LN, NL) fits this one AIR id at any log_n >= 5.  Every constraint has degree <= 3.
// Public inputs (24): NL, NL + FB, w^-1 (w = the 2^LN-th root of unity: the only per-table constant), TREE0 (below), beta_l for
// eight layers (zero behind NL; NL <= 8 covers every LDE up to 2^27 at this arity) and the CLAIMS DIGEST, hash_n_to_hash_no_pad
// of the list (index, ev_0, leaf_0 .. leaf_(NL-1)) of all queries in order.  The table does not constrain the digest: it is a
// public input so that the lookup challenges depend on the claims (as in MerkleOpenAir / LeafSpongeAir).
// Bus: a fold row RECEIVES the 32 words of its leaf as TAG_ROW messages (leaf index Q, position, word, tree = TREE0 + layer) --
// what a LeafSpongeAir over the layer trees sends (with TREE0 = 0 and one layer that is the message LeafSpongeAir sends today);
// a query's first row RECEIVES the TAG_FRI message (index, ev_0, 0) and its first bit row SENDS (index, ev_NL, 1).  34 messages,
// two per extension helper; one cyclic running sum; the table publishes total / rows.
// Constraint ORDER is protocol: tests/fri_fold_ref.py restates it independently.
#pragma once
#include <vector>

#include "air.cuh"

namespace ffa {
constexpr int ACT = 0, FOLD = 1, FIRST = 2, LAST = 3, FBIT = 4, CNT = 5, R = 6, Q = 7, IDX = 8, B = 9, OH = 13, LSEL = 29;
constexpr int Y = 37, SI = 38, Y0 = 42, A = 43, BE = 48, EV = 56, LEAF = 58, V1 = 90, V2 = 106, V3 = 114, V4 = 118, COLS = 120;
constexpr int N_HELP = 17, AUX = 2 * N_HELP + 2, MAX_LAYERS = 8;
constexpr int PUB_NL = 0, PUB_ROWS = 1, PUB_WINV = 2, PUB_TREE0 = 3, PUB_BETA = 4, PUB_DIGEST = 20, PUB = 24;

constexpr uint64_t cmul(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) % GL_P); }
constexpr uint64_t cpow(uint64_t a, uint64_t e) {
    uint64_t r = 1;
    for (; e; e >>= 1, a = cmul(a, a))
        if (e & 1) r = cmul(r, a);
    return r;
}
constexpr int cbrev(int x, int bits) {
    int r = 0;
    for (int i = 0; i < bits; ++i) r = (r << 1) | ((x >> i) & 1);
    return r;
}
constexpr uint64_t G16 = cpow(1753635133440165772ULL, (uint64_t)1 << 28);  // the 16th root of unity: 7^((p-1)/2^32) raised to 2^28
constexpr uint64_t HALF = cpow(2, GL_P - 2), INV7 = cpow(7, GL_P - 2);
static_assert(cpow(G16, 8) == GL_P - 1 && cmul(HALF, 2) == 1 && cmul(INV7, 7) == 1, "air_fri_fold.cuh: constants");
// gp[t] = g^bitrev(t, 4): the factor between 1 / x and the inverse of the coset base, by the leaf slot of x;
// fc[level j][pair k] = 1 / (2 g^(2^j bitrev(k, 3 - j))): pair k of level j sits at base^(2^j) times that power of g
struct Tab {
    uint64_t gp[16], fc[4][8];
};
constexpr Tab make_tab() {
    Tab t{};
    for (int i = 0; i < 16; ++i) t.gp[i] = cpow(G16, (uint64_t)cbrev(i, 4));
    for (int j = 0; j < 4; ++j)
        for (int k = 0; k < (8 >> j); ++k) t.fc[j][k] = cmul(HALF, cpow(G16, (uint64_t)((16 - (1 << j) * cbrev(k, 3 - j)) % 16)));
    return t;
}
constexpr int vlev(int j) { return j == 0 ? LEAF : j == 1 ? V1 : j == 2 ? V2 : j == 3 ? V3 : V4; }
}  // namespace ffa

struct FriFoldAir {
    static constexpr int ID = 18, COLS = ffa::COLS, PUB = ffa::PUB, PERIODIC = 0, PERIOD_LOG = 0, QUOT_ROWS_PER_LANE = 1, AUX = ffa::AUX, CHAL = 4, AUXPUB = 1, EXACT_LOG = 0;
    static constexpr int plog(int) { return 0; }
    static int32_t gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub);
    static void periodic_values(std::vector<uint64_t>& v) { v.clear(); }

    static constexpr int N_HELP = ffa::N_HELP, BUS_ROWS = 1, BUS_STEP = -1, BUS_BLOCK = 64, BUS_PERIODIC = 0;

    // 32 leaf words received on a fold row; the entry received on the first row, the exit sent on the first bit row
    template <class F, class Row, class Sink>
    VX_HD static void messages(const Row& loc, const F*, const F* pub, const bus::Bus<X2<F>>& bus, Sink& s) {
        using namespace ffa;
        const F zero = F::from(0), tree = pub[PUB_TREE0] + loc[CNT], q = loc[Q], idx = loc[IDX], received = zero - loc[FOLD];
#pragma unroll Sink::UNROLL
        for (int e = 0; e < 16; ++e)
            s.pair(received, bus.row_of(tree, q, F::from((uint64_t)(2 * e)), loc[LEAF + 2 * e]), bus.row_of(tree, q, F::from((uint64_t)(2 * e + 1)), loc[LEAF + 2 * e + 1]));
        s.put(zero - loc[FIRST], bus.fri(idx, loc[EV], loc[EV + 1], bus::K<0>{}), loc[FBIT], bus.fri(idx, loc[EV], loc[EV + 1], bus::K<1>{}));
    }

    template <class F, class Row, class Cn>
    __host__ __device__ static void eval(const Row& loc, const Row& nxt, const F*, const F* pub, const F* chal, const F* apub, Cn& c) {
        using namespace ffa;
        constexpr Tab T = make_tab();
        const F one = F::from(1), zero = F::from(0);
        const F act = loc[ACT], fold = loc[FOLD], first = loc[FIRST], last = loc[LAST], cnt = loc[CNT], r = loc[R], q = loc[Q], idx = loc[IDX], cont = act - last;
        // ---- 1. boolean cells
        c.constraint(act * (act - one));
        c.constraint(fold * (fold - one));
        c.constraint(last * (last - one));
#pragma unroll 1
        for (int j = B; j < LSEL + MAX_LAYERS; ++j) c.constraint(loc[j] * (loc[j] - one));  // the bits, both one-hots
        // ---- 2. the shape of a query: fold rows, then bit rows
        c.constraint(fold * (one - act));
        c.constraint(last * (one - act));
        c.constraint(last * fold);
#pragma unroll 1
        for (int i = 1; i < 4; ++i) c.constraint((act - fold) * loc[B + i]);
        c.constraint(first * (one - fold));
        c.constraint(nxt[FIRST] - nxt[ACT] * (one - cont));
        c.constraint(nxt[FBIT] - fold * (one - nxt[FOLD]));
        c.constraint(nxt[FOLD] * (one - nxt[FIRST]) * (one - fold));
        c.constraint(fold * (one - nxt[FOLD]) * (cnt + one - pub[PUB_NL]));
        c.constraint(cont * (one - nxt[ACT]));
        // ---- 3. the row counter and the index digits
        const F b0 = loc[B], b1 = loc[B + 1], b2 = loc[B + 2], b3 = loc[B + 3];
        const F within = b0 + b1 * F::from(2) + b2 * F::from(4) + b3 * F::from(8);
        c.constraint(first * cnt);
        c.constraint(cont * (nxt[CNT] - cnt - one));
        c.constraint(last * (cnt + one - pub[PUB_ROWS]));
        c.constraint(r - within - q * (fold * F::from(14) + F::from(2)));
        c.constraint(cont * (nxt[R] - q));
        c.constraint(last * q);
        c.constraint(first * (r - idx));
        c.constraint(cont * (nxt[IDX] - idx));
        // ---- 4. the one-hots: of `within` on a fold row, of the layer (= the counter) on a fold row; all zero elsewhere
        F gsum = zero;  // sum over the one-hot of g^bitrev(t): the factor of the coset base
        {
            F s0 = zero, s1 = zero;
#pragma unroll 1
            for (int t = 0; t < 16; ++t) {
                const F o = loc[OH + t];
                s0 = s0 + o, s1 = s1 + o * F::from((uint64_t)t), gsum = gsum + o * F::from(T.gp[t]);
            }
            c.constraint(s0 - fold);
            c.constraint(s1 - fold * within);
            s0 = zero, s1 = zero;
#pragma unroll 1
            for (int i = 0; i < MAX_LAYERS; ++i) s0 = s0 + loc[LSEL + i], s1 = s1 + loc[LSEL + i] * F::from((uint64_t)i);
            c.constraint(s0 - fold);
            c.constraint(s1 - fold * cnt);
        }
        // ---- 5. the point, by inverses
        const F y = loc[Y], y0 = loc[Y0];
        c.constraint(loc[SI] - y * gsum);
#pragma unroll 1
        for (int j = 0; j < 3; ++j) c.constraint(loc[SI + j + 1] - loc[SI + j] * loc[SI + j]);
        c.constraint(fold * (nxt[Y] - loc[SI + 3] * loc[SI + 3]));
        c.constraint(first * (y - y0));
        c.constraint(cont * (nxt[Y0] - y0));
        // ---- 6. 1 / x_0 is bound to the index: square and multiply over the bits
        {
            const F wm1 = pub[PUB_WINV] - one;
            c.constraint(first * (loc[A] - one));
#pragma unroll 1
            for (int i = 0; i < 4; ++i) c.constraint(loc[A + i + 1] - loc[A + i] * loc[A + i] * (loc[B + i] * wm1 + one));
            c.constraint(cont * (nxt[A] - loc[A + 1] - fold * (loc[A + 4] - loc[A + 1])));
            c.constraint(last * (y0 - loc[A + 1] * F::from(INV7)));
        }
        // ---- 7. beta_l (picked by the layer one-hot) and its squares
        {
            X2<F> bl{zero, zero};
#pragma unroll 1
            for (int i = 0; i < MAX_LAYERS; ++i) bl = bl + X2<F>{pub[PUB_BETA + 2 * i], pub[PUB_BETA + 2 * i + 1]} * loc[LSEL + i];
            c.constraint_x2(X2<F>{loc[BE], loc[BE + 1]} - bl);
#pragma unroll 1
            for (int j = 0; j < 3; ++j) {
                const X2<F> bj{loc[BE + 2 * j], loc[BE + 2 * j + 1]};
                c.constraint_x2(X2<F>{loc[BE + 2 * j + 2], loc[BE + 2 * j + 3]} - bj * bj);
            }
        }
        // ---- 8. the value entering the layer is the leaf's slot `within`; the value leaving it enters the next row
        {
            X2<F> pick{zero, zero};
#pragma unroll 1
            for (int t = 0; t < 16; ++t) pick = pick + X2<F>{loc[LEAF + 2 * t], loc[LEAF + 2 * t + 1]} * loc[OH + t];
            c.constraint_x2(pick - X2<F>{loc[EV], loc[EV + 1]} * fold);
            c.constraint_x2((X2<F>{nxt[EV], nxt[EV + 1]} - X2<F>{loc[V4], loc[V4 + 1]}) * fold);
        }
        // ---- 9. the fold: four arity-2 levels, 8 + 4 + 2 + 1 pairs
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const X2<F> bj{loc[BE + 2 * j], loc[BE + 2 * j + 1]};
            const F sj = loc[SI + j];
#pragma unroll 1
            for (int k = 0; k < (8 >> j); ++k) {
                const int in = vlev(j) + 4 * k, out = vlev(j + 1) + 2 * k;
                const X2<F> u{loc[in], loc[in + 1]}, w{loc[in + 2], loc[in + 3]};
                c.constraint_x2(X2<F>{loc[out], loc[out + 1]} - (u + w) * F::from(HALF) - bj * (u - w) * (sj * F::from(T.fc[j][k])));
            }
        }
        // ---- 10. the bus (messages above): two messages per helper, the running sum advances on every row
        bus_constraints<FriFoldAir>(loc, nxt, (const F*)nullptr, pub, chal, apub, c);
    }
};
