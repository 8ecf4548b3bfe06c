// FriCombineAir (AIR id 21): the FRI combination of every query of one inner proof in one table -- what vx_stark_verify_ext does
// per query before the fold loop (vx_verify.hip: "reduced openings" and the loop over the opened rows; plonky2 v0.2.0
// fri/verifier.rs fri_combine_initial), the fourth table of proof aggregation.  For an inner proof with an LDE of 2^LN points, cm
// main, ca auxiliary (may be 0) and nq quotient columns, c = cm + ca, the challenge alpha, the point zeta, zeta' = zeta w_n and the
// reduced openings y0, y1, a query (index, row words w_0 .. w_(c+nq-1)) is c + nq ABSORB rows followed by LN BIT rows:
//   absorb row j  holds ONE word W = w_j, its tree as a three-way selector (TM main / TA auxiliary / TQ quotient), its position POS
//                 in that tree's row, the power AP = alpha^j (1 on the query's first row, next AP = AP alpha, running on across
//                 the trees) and the sum S = previous S + AP W; S1, constant over the query, equals S on the last non-quotient
//                 absorb row.  A tree may end only where POS + 1 is its public length, main is followed by auxiliary unless
//                 ca = 0, auxiliary by quotient, quotient by the bit rows
//   bit row       carries S and S1 on and consumes one index bit, LSB first: R = 2 Q + B, next R = Q, R = IDX on the first bit row
//                 and Q = 0 on the query's last row (the closing rule of FriFoldAir: without it a wrong bit could be hidden by
//                 continuing R with field divisions).  The accumulator A starts at 1 and A1 = A^2 w^B enters the next row: MSB-
//                 first exponentiation by bitrev(index, LN).  A row counter CNT runs from 0 over the query and closes on the
//                 public row count, so there are exactly LN bit rows
//   the last row  holds x = 7 A1 (an expression, no column), D0 = 1 / (x - zeta), D1 = 1 / (x - zeta') and
//                 EV = alpha^c (S - y0) D0 + (S1 - y1) D1 = ev_0.  x is carried forward, not by inverses as in FriFoldAir: the two
//                 extension inverses D0, D1 are needed either way and 1 / x would add a third
// One word per absorb row: no tail flags, no per-row word count, and every rule below has degree <= 3.  The queries follow each
// other and idle rows (all zero) fill the rest.  Nothing is positional: every constraint holds on every row pair, the wrap-around
// included, there are no first-row or last-row constraints and no periodic columns, so any number of queries of any shape
// (LN, cm, ca, nq) fits this one AIR id at any log_n >= 5.
// Public inputs (22): rows per query, cm, ca, nq, TREE0, w (the 2^LN-th root of unity), alpha, alpha^c, zeta, zeta', y0, y1 and
// four digest words the table does not constrain (they make the lookup challenges depend on the claims).  The verifier rebuilds
// every one, so the table proves neither alpha^c nor y0.
// Bus: every absorb row RECEIVES row_of(TREE0 + t, IDX, POS, W), t = 0 main / 1 auxiliary / 2 quotient -- what a leaf sponge over
// the commitment trees sends; the query's last row SENDS fri(IDX, EV, 0), the entry FriFoldAir receives.  No row does both, so
// ONE helper carries both messages; one cyclic running sum; the table publishes total / rows.
// Constraint ORDER is protocol: tests/fri_combine_ref.py restates it independently.
#pragma once
#include <vector>

#include "air.cuh"

namespace fca {
constexpr int ACT = 0, TM = 1, TA = 2, TQ = 3, FIRST = 4, LAST = 5, FBIT = 6, CNT = 7, POS = 8, W = 9, IDX = 10, R = 11, Q = 12, B = 13, A = 14, A1 = 15;
constexpr int AP = 16, S = 18, S1 = 20, D0 = 22, D1 = 24, EV = 26, COLS = 28;
constexpr int N_HELP = 1, AUX = 2 * N_HELP + 2;
constexpr int PUB_ROWS = 0, PUB_CM = 1, PUB_CA = 2, PUB_NQ = 3, PUB_TREE0 = 4, PUB_W = 5, PUB_ALPHA = 6, PUB_ALPHAC = 8, PUB_ZETA = 10, PUB_ZETAN = 12, PUB_Y0 = 14, PUB_Y1 = 16;
constexpr int PUB_DIGEST = 18, PUB = 22;
constexpr uint64_t TREE0 = 8;  // the commitment trees of vx_fri_combine_prove: behind FriFoldAir's layer ids (ffa::MAX_LAYERS)
}  // namespace fca

struct FriCombineAir {
    static constexpr int ID = 21, COLS = fca::COLS, PUB = fca::PUB, PERIODIC = 0, PERIOD_LOG = 0, QUOT_ROWS_PER_LANE = 1, AUX = fca::AUX, CHAL = 4, AUXPUB = 1, EXACT_LOG = 0;
    static constexpr int plog(int) { return 0; }
    static int32_t gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub);
    static void periodic_values(std::vector<uint64_t>& v) { v.clear(); }

    static constexpr int N_HELP = fca::N_HELP, BUS_ROWS = 1, BUS_STEP = -1, BUS_BLOCK = 256, BUS_PERIODIC = 0;

    // a row word received on an absorb row, the entry of the fold chain sent on the last row
    template <class F, class Row, class Sink>
    VX_HD static void messages(const Row& loc, const F*, const F* pub, const bus::Bus<X2<F>>& bus, Sink& s) {
        using namespace fca;
        const F ta = loc[TA], tq = loc[TQ], idx = loc[IDX];
        s.put(F::from(0) - (loc[TM] + ta + tq), bus.row_of(pub[PUB_TREE0] + ta + tq + tq, idx, loc[POS], loc[W]), loc[LAST], bus.fri(idx, loc[EV], loc[EV + 1], bus::K<0>{}));
    }

    template <class F, class Row, class Cn>
    __host__ __device__ static void eval(const Row& loc, const Row& nxt, const F*, const F* pub, const F* chal, const F* apub, Cn& c) {
        using namespace fca;
        const F one = F::from(1);
        const F act = loc[ACT], tm = loc[TM], ta = loc[TA], tq = loc[TQ], first = loc[FIRST], last = loc[LAST], fbit = loc[FBIT], cnt = loc[CNT], pos = loc[POS], w = loc[W];
        const F idx = loc[IDX], r = loc[R], q = loc[Q], b = loc[B], a = loc[A], a1 = loc[A1];
        const F abs = tm + ta + tq, bit = act - abs, cont = act - last, nabs = nxt[TM] + nxt[TA] + nxt[TQ];
        // ---- 1. boolean cells; at most one tree
        c.constraint(act * (act - one));
        c.constraint(tm * (tm - one));
        c.constraint(ta * (ta - one));
        c.constraint(tq * (tq - one));
        c.constraint(abs * (abs - one));
        c.constraint(last * (last - one));
        c.constraint(b * (b - one));
        // ---- 2. the shape of a query: main, auxiliary (unless ca = 0), quotient, then bit rows up to the last row
        c.constraint(abs * (one - act));
        c.constraint(last * (one - act));
        c.constraint(last * abs);
        c.constraint(first * (one - tm));
        c.constraint(nxt[FIRST] - nxt[ACT] * (one - cont));
        c.constraint(nxt[FBIT] - abs * (one - nabs));
        c.constraint(cont * (one - nxt[ACT]));
        c.constraint(tm * (one - nabs));
        c.constraint(ta * (one - nxt[TA] - nxt[TQ]));
        c.constraint(nxt[TM] * (one - nxt[FIRST]) * (one - tm));
        c.constraint(nxt[TA] * (one - tm - ta));
        c.constraint(nxt[TQ] * (one - abs));
        c.constraint(bit * cont * nabs);
        c.constraint(tm * nxt[TQ] * pub[PUB_CA]);
        // ---- 3. a tree ends only at its public length; POS starts at 0 in each tree and counts up
        c.constraint(tm * (one - nxt[TM]) * (pos + one - pub[PUB_CM]));
        c.constraint(ta * (one - nxt[TA]) * (pos + one - pub[PUB_CA]));
        c.constraint(tq * (one - nxt[TQ]) * (pos + one - pub[PUB_NQ]));
        {
            const F same = tm * nxt[TM] + ta * nxt[TA] + tq * nxt[TQ];
            c.constraint(same * (nxt[POS] - pos - one));
            c.constraint((nabs - same) * nxt[POS]);
        }
        // ---- 4. the row counter closes on the public row count
        c.constraint(first * cnt);
        c.constraint(cont * (nxt[CNT] - cnt - one));
        c.constraint(last * (cnt + one - pub[PUB_ROWS]));
        // ---- 5. the word, the power of alpha, the sums
        const X2<F> ap{loc[AP], loc[AP + 1]}, s{loc[S], loc[S + 1]}, s1{loc[S1], loc[S1 + 1]};
        {
            const X2<F> nap{nxt[AP], nxt[AP + 1]}, alpha{pub[PUB_ALPHA], pub[PUB_ALPHA + 1]};
            c.constraint(bit * w);
            c.constraint_x2((ap - one) * first);
            c.constraint_x2((nap - ap * alpha) * (abs * nabs));
            c.constraint_x2((s - w) * first);
            c.constraint_x2((X2<F>{nxt[S], nxt[S + 1]} - s - nap * nxt[W]) * cont);
            c.constraint_x2((X2<F>{nxt[S1], nxt[S1 + 1]} - s1) * cont);
            c.constraint_x2((s - s1) * ((tm + ta) * nxt[TQ]));
        }
        // ---- 6. the index bits, LSB first; the query's last row leaves none
        c.constraint(r - q - q - b);
        c.constraint(bit * cont * (nxt[R] - q));
        c.constraint(last * q);
        c.constraint(fbit * (r - idx));
        c.constraint(cont * (nxt[IDX] - idx));
        // ---- 7. x_0 is bound to the index: square and multiply over the bits
        c.constraint(fbit * (a - one));
        c.constraint(a1 - a * a * (b * (pub[PUB_W] - one) + one));
        c.constraint(bit * cont * (nxt[A] - a1));
        // ---- 8. the last row: the two inverses and ev_0
        const X2<F> ev{loc[EV], loc[EV + 1]};
        {
            const F x = a1 * F::from(7);
            const X2<F> d0{loc[D0], loc[D0 + 1]}, d1{loc[D1], loc[D1 + 1]}, zeta{pub[PUB_ZETA], pub[PUB_ZETA + 1]}, zetan{pub[PUB_ZETAN], pub[PUB_ZETAN + 1]};
            const X2<F> alphac{pub[PUB_ALPHAC], pub[PUB_ALPHAC + 1]}, y0{pub[PUB_Y0], pub[PUB_Y0 + 1]}, y1{pub[PUB_Y1], pub[PUB_Y1 + 1]};
            const X2<F> xz{x - zeta.a, F::from(0) - zeta.b}, xzn{x - zetan.a, F::from(0) - zetan.b};
            c.constraint_x2((d0 * xz - one) * last);
            c.constraint_x2((d1 * xzn - one) * last);
            c.constraint_x2((ev - alphac * (s - y0) * d0 - (s1 - y1) * d1) * last);
        }
        // ---- 9. the bus (messages above): no row does both, so one helper carries both messages
        bus_constraints<FriCombineAir>(loc, nxt, (const F*)nullptr, pub, chal, apub, c);
    }
};
