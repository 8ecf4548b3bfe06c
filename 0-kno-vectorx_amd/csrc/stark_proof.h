// The VXSTARK1 proof and its Fiat-Shamir transcript, stated ONCE for the prover (vx_stark.hip), the verifier (vx_verify.hip) and
// every other reader: where each word of a proof sits (Shape, Proof), in which order the transcript absorbs them and what it
// yields (Transcript), and the values both sides derive from the openings (reduce_openings).  Header-only standard C++.
//
// Layout: 10 header words (magic, AIR id, degree bits, main columns, quotient columns, rate_bits, cap_height, num_queries, pow_bits,
// FRI layers), the arity bits of every layer, the length of the final polynomial, the number of public inputs; the public inputs;
// the trace cap; [published values, auxiliary cap]; the quotient cap; the openings at zeta (local), zeta w (next) and of the
// quotient chunks; one cap per FRI layer; the final polynomial; the proof-of-work nonce; one record per query (Query).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#pragma GCC visibility push(default)
#include "../../include/vx.h"
#pragma GCC visibility pop
#include "glh_poseidon.h"

namespace stark_proof {
static const uint64_t MAGIC = 0x314b524154535856ULL;  // "VXSTARK1"
static constexpr size_t NQ = 4;  // quotient columns: quotient_degree_factor 2 (constraint degree 3), 2 challenges

// the configuration steers loops on both sides (a circuit.json can carry it)
inline bool config_ok(const vx_stark_config& c) {
    return c.rate_bits >= 1 && c.rate_bits <= 3 && c.arity_bits >= 1 && c.arity_bits <= 5 && c.final_poly_bits >= 0 && c.final_poly_bits <= 27 &&
           c.num_queries >= 1 && c.num_queries <= 1024 && c.pow_bits >= 0 && c.pow_bits <= 32 && c.cap_height >= 0 && c.cap_height <= 27;
}
// FriReductionStrategy::ConstantArityBits(arity_bits, final_poly_bits): no layer's tree is lower than the cap
inline std::vector<int> fri_arity_plan(int degree_bits, const vx_stark_config& cfg) {
    std::vector<int> r;
    for (int d = degree_bits; d > cfg.final_poly_bits && d + cfg.rate_bits - cfg.arity_bits >= cfg.cap_height; d -= cfg.arity_bits) r.push_back(cfg.arity_bits);
    return r;
}

// Everything the length and the offsets of a proof depend on.  L and cfg must be in range: 2 <= L <= 26, config_ok(cfg) and
// cap_height <= L + rate_bits (then no Merkle depth is negative: the arity plan keeps every layer's tree above the cap).
struct Shape {
    int air_id, L, r, cap_h, num_queries, pow_bits, LN, depth0;  // depth0: siblings of a path in the trace / auxiliary / quotient tree
    size_t cm, ca, c, n_pub, auxpub, cap_words, final_len;       // c = cm + ca committed trace columns; auxpub: published X2 values
    std::vector<int> arities, depth;                             // per FRI layer: arity bits, siblings of a path in its tree
    std::vector<size_t> q_layer;                                 // per FRI layer: where its words start in a query record
    size_t o_pub, o_cap_trace, o_apub, o_cap_aux, o_cap_quot, o_local, o_next, o_quot, o_layer_caps, o_final, o_nonce, o_queries;
    size_t q_sib_t, q_row_a, q_sib_a, q_row_q, q_sib_q, q_words;  // inside a query record (row_t at 0)
    size_t n_words;
    Shape(int air_id_, size_t cm_, size_t ca_, size_t n_pub_, size_t auxpub_, int L_, const vx_stark_config& cfg)
        : air_id(air_id_), L(L_), r(cfg.rate_bits), cap_h(cfg.cap_height), num_queries(cfg.num_queries), pow_bits(cfg.pow_bits), LN(L_ + cfg.rate_bits),
          depth0(LN - cap_h), cm(cm_), ca(ca_), c(cm_ + ca_), n_pub(n_pub_), auxpub(auxpub_), cap_words((size_t)4 << cap_h), arities(fri_arity_plan(L_, cfg)) {
        size_t at = 12 + arities.size();
        auto take = [&at](size_t n) { return (at += n) - n; };
        o_pub = take(n_pub), o_cap_trace = take(cap_words);
        o_apub = take(ca ? 2 * auxpub : 0), o_cap_aux = take(ca ? cap_words : 0);
        o_cap_quot = take(cap_words), o_local = take(2 * c), o_next = take(2 * c), o_quot = take(2 * NQ);
        o_layer_caps = take(arities.size() * cap_words);
        at = 0;  // the query record: three rows with their paths, then per layer the other evaluations of the coset and a path
        take(cm), q_sib_t = take(4 * (size_t)depth0), q_row_a = take(ca), q_sib_a = take(ca ? 4 * (size_t)depth0 : 0);
        q_row_q = take(NQ), q_sib_q = take(4 * (size_t)depth0);
        int cur = LN;
        for (int a : arities) {
            cur -= a;
            depth.push_back(cur - cap_h);
            q_layer.push_back(take(2 * (((size_t)1 << a) - 1) + 4 * (size_t)(cur - cap_h)));
        }
        q_words = at;
        final_len = ((size_t)1 << cur) >> r;
        at = o_layer_caps + arities.size() * cap_words;
        o_final = take(2 * final_len), o_nonce = take(1), o_queries = take((size_t)num_queries * q_words);
        n_words = at;
    }
    std::vector<uint64_t> header_words() const {
        std::vector<uint64_t> h{MAGIC, (uint64_t)air_id, (uint64_t)L, cm, NQ, (uint64_t)r, (uint64_t)cap_h, (uint64_t)num_queries, (uint64_t)pow_bits, arities.size()};
        h.insert(h.end(), arities.begin(), arities.end());
        h.push_back(final_len), h.push_back(n_pub);
        return h;
    }
    size_t query_words() const { return q_words; }
    size_t words() const { return n_words; }  // the exact length of a proof
    // what callers size their buffers by before proving: a little above words() (paths counted from the leaves to the root)
    size_t bound_words() const {
        const size_t n_layers = arities.size();
        size_t per_query = c + NQ + 2 * 4 * (size_t)LN, w = 16 + n_layers + n_pub + 2 * cap_words + 2 * (2 * c + NQ) + n_layers * cap_words + 1;
        if (ca) per_query += 4 * (size_t)LN, w += cap_words + 2 * auxpub;
        size_t cur = LN;
        for (int a : arities) per_query += 2 * (((size_t)1 << a) - 1) + 4 * cur, cur -= a;
        return w + 2 * final_len + (size_t)num_queries * per_query;
    }
};

// One query of a proof: the opened rows of the three trees, each followed by its path (4 depth0 words); per FRI layer the
// 2 (arity - 1) words of the coset's other evaluations, followed by the path in that layer's tree (4 depth[l] words).
template <class W>
struct Query {
    W* p;
    const Shape* s;
    W* row_t() const { return p; }
    W* sib_t() const { return p + s->q_sib_t; }
    W* row_a() const { return p + s->q_row_a; }
    W* sib_a() const { return p + s->q_sib_a; }
    W* row_q() const { return p + s->q_row_q; }
    W* sib_q() const { return p + s->q_sib_q; }
    W* evals(size_t l) const { return p + s->q_layer[l]; }
    W* sibs(size_t l) const { return evals(l) + 2 * (((size_t)1 << s->arities[l]) - 1); }
};
// A proof of a shape, its sections by name: W = uint64_t for the prover, which writes them (Writer), const uint64_t for a reader (View).
template <class W>
struct Proof {
    W* pr = nullptr;
    const Shape* s = nullptr;
    W* pub() const { return pr + s->o_pub; }
    W* cap_trace() const { return pr + s->o_cap_trace; }
    W* apub() const { return pr + s->o_apub; }  // 2 auxpub words; with cap_aux only present when the AIR has auxiliary columns
    W* cap_aux() const { return pr + s->o_cap_aux; }
    W* cap_quot() const { return pr + s->o_cap_quot; }
    W* open_local() const { return pr + s->o_local; }  // 2 c words
    W* open_next() const { return pr + s->o_next; }
    W* open_quot() const { return pr + s->o_quot; }    // 2 NQ words
    W* layer_cap(size_t l) const { return pr + s->o_layer_caps + l * s->cap_words; }
    W* final_poly() const { return pr + s->o_final; }  // 2 final_len words
    W* nonce() const { return pr + s->o_nonce; }
    Query<W> query(size_t k) const { return {pr + s->o_queries + k * s->q_words, s}; }
};
struct View : Proof<const uint64_t> {
    // nullptr and a view of the `len` words at pr, or what is wrong with them: the first section they do not hold.  Bounds are checked here, once:
    // a view only exists over exactly shape.words() words.
    static const char* parse(const uint64_t* pr, size_t len, const Shape& shape, View* out) {
        if (len < shape.o_pub) return "proof truncated (header)";
        if (len < shape.o_cap_trace) return "proof truncated (public inputs)";
        if (len < shape.o_layer_caps) return "proof truncated (caps/openings)";
        if (len < shape.o_final) return "proof truncated (FRI caps)";
        if (len < shape.o_queries) return "proof truncated (final poly)";
        if (len < shape.words()) return "proof truncated (queries)";
        if (len != shape.words()) return "trailing data in proof";
        out->pr = pr, out->s = &shape;
        return nullptr;
    }
    // ... of the HEAD of a proof, everything before the query records: for a reader that never calls query().  The words are the
    // whole proof (the records are there and are not read) or the head alone; no other length is a proof of this shape.
    static const char* parse_head(const uint64_t* pr, size_t len, const Shape& shape, View* out) {
        if (len != shape.o_queries) return parse(pr, len, shape, out);
        out->pr = pr, out->s = &shape;
        return nullptr;
    }
};
struct Writer : Proof<uint64_t> {
    std::vector<uint64_t> words;
    Writer(const Shape& shape, const uint64_t* public_inputs) : words(shape.words()) {
        pr = words.data(), s = &shape;
        const std::vector<uint64_t> h = shape.header_words();
        std::copy(h.begin(), h.end(), words.begin());
        std::copy(public_inputs, public_inputs + shape.n_pub, pub());
    }
};

// The transcript: one method per protocol step, in the order both sides call them (plonky2 iop/challenger.rs, starky prover.rs).
// Stated over the challenger C: glh::Challenger hashes (prover and verifier), glh::RecordingChallenger hashes and keeps what
// TranscriptAir proves of it, glh::ClaimedChallenger hashes nothing and answers with claimed challenges (vx_stark_transcripts_verify).
template <class C>
struct TranscriptOf : C {
    using C::challenge;
    using C::observe;
    Fx ext() {
        const uint64_t a = challenge(), b = challenge();
        return {a, b};
    }
    template <class W>
    void trace(const Proof<W>& p) { observe(p.pub(), p.s->n_pub), observe(p.cap_trace(), p.s->cap_words); }
    // lookup challenges after the trace cap: drawn, or -- SHARED with the other tables of a bus -- given and absorbed, so that everything
    // after depends on them
    void lookup_challenges(uint64_t* out, size_t n, const uint64_t* external) {
        for (size_t q = 0; q < n; ++q) out[q] = external ? external[q] : challenge();
        if (external) observe(out, n);
    }
    template <class W>
    void aux(const Proof<W>& p) { observe(p.apub(), 2 * p.s->auxpub), observe(p.cap_aux(), p.s->cap_words); }
    void alphas(uint64_t out[2]) { out[0] = challenge(), out[1] = challenge(); }
    template <class W>
    Fx zeta(const Proof<W>& p) { return observe(p.cap_quot(), p.s->cap_words), ext(); }
    template <class W>
    Fx alpha(const Proof<W>& p) {  // challenger.observe_openings: batch 0 = local ++ quotient, batch 1 = next
        observe(p.open_local(), 2 * p.s->c), observe(p.open_quot(), 2 * NQ), observe(p.open_next(), 2 * p.s->c);
        return ext();
    }
    template <class W>
    Fx beta(const Proof<W>& p, size_t l) { return observe(p.layer_cap(l), p.s->cap_words), ext(); }
    template <class W>
    void final_poly(const Proof<W>& p) { observe(p.final_poly(), 2 * p.s->final_len); }
    // the sponge state the proof of work grinds on: a nonce absorbed at position n_in must make pow_ok
    int grind_state(uint64_t st_out[12]) const {
        memcpy(st_out, this->st, sizeof this->st);
        memcpy(st_out, this->in, this->n_in * 8);
        return this->n_in;
    }
    bool pow_ok(uint64_t nonce, int pow_bits) {
        observe(nonce);
        const uint64_t resp = challenge();
        return pow_bits == 0 || (resp >> (64 - pow_bits)) == 0;
    }
    size_t query_index(size_t N) { return challenge() % N; }
};
using Transcript = TranscriptOf<glh::Challenger>;

// Lookup challenges shared by the k tables of a bus: a transcript of every table's public inputs and trace cap, in bus order.
inline void shared_challenges_n(const uint64_t* const* pubs, const size_t* n_pubs, const uint64_t* const* caps, size_t k, size_t cap_words, uint64_t* out, size_t n_out) {
    glh::Challenger sc;
    for (size_t t = 0; t < k; ++t) sc.observe(pubs[t], n_pubs[t]), sc.observe(caps[t], cap_words);
    for (size_t q = 0; q < n_out; ++q) out[q] = sc.challenge();
}
// (public inputs, trace cap) of a serialised proof whose AIR is not known yet, for deriving shared challenges; false if too short
inline bool peek(const uint64_t* pr, size_t len, int cap_height, const uint64_t** pub, size_t* n_pub, const uint64_t** cap) {
    if (len < 12 || pr[9] > 16) return false;
    const size_t o_pub = 12 + pr[9], np = o_pub <= len ? pr[o_pub - 1] : 65;  // Shape::o_pub, header_words().back()
    if (np > 64 || cap_height < 0 || cap_height > 16 || o_pub + np + ((size_t)4 << cap_height) > len) return false;
    *pub = pr + o_pub, *n_pub = np, *cap = pr + o_pub + np;
    return true;
}

// What the query phase and every party outside a table of it derive from an index: the low `bits` bits of x reversed, the point of
// a query index on the LDE coset, 7 w_LN^brev(index), and the value of a final polynomial given as word pairs at a base-field point.
inline size_t brev(size_t x, int bits) {
    size_t r = 0;
    for (int i = 0; i < bits; ++i) r = (r << 1) | ((x >> i) & 1);
    return r;
}
inline uint64_t query_point(uint64_t index, int LN) { return glh::mul(7, glh::pow(glh::root(LN), brev(index, LN))); }
inline Fx final_poly_at(const uint64_t* final_poly, size_t final_len, uint64_t x) {
    Fx fp{0, 0};
    for (size_t k = final_len; k-- > 0;) fp = fp * Fx{x, 0} + Fx{final_poly[2 * k], final_poly[2 * k + 1]};
    return fp;
}

// fri_combine_initial's reduced openings: with the c trace columns' openings at zeta (local) and zeta w (next) and the nq quotient
// openings at zeta, as word pairs, y0 = sum_j alpha^j (local ++ quot)[j], y1 = sum_j alpha^j next[j].  apow (optional) receives
// alpha^0 .. alpha^(c + nq - 1) as word pairs.
struct Reduced {
    Fx y0, y1, alpha_c;
};
inline Reduced reduce_openings(Fx alpha, const uint64_t* local, const uint64_t* next, const uint64_t* quot, size_t c, size_t nq, uint64_t* apow = nullptr) {
    Reduced r{{0, 0}, {0, 0}, {1, 0}};
    Fx ap{1, 0};
    for (size_t j = 0; j < c + nq; ++j, ap = ap * alpha) {
        if (j == c) r.alpha_c = ap;
        if (apow) apow[2 * j] = ap.a, apow[2 * j + 1] = ap.b;
        const uint64_t* o = j < c ? local + 2 * j : quot + 2 * (j - c);
        r.y0 = r.y0 + ap * Fx{o[0], o[1]};
        if (j < c) r.y1 = r.y1 + ap * Fx{next[2 * j], next[2 * j + 1]};
    }
    if (nq == 0) r.alpha_c = ap;
    return r;
}
}  // namespace stark_proof
