// The statement of the VXSTARK1 proof layout and transcript (0-kno-vectorx_amd/csrc/stark_proof.h) driven on a CPU over a grid of
// shapes.  The layout is restated here ONCE more, as the order in which `sections` visits a proof: a proof of counter words written
// through Writer in that order must be the counter itself (the sections tile the proof, in order, without gap or overlap), View must
// hand the same words back, every strict prefix must be refused, the transcript must reach the same query indices in the prover's
// and in the verifier's call order, and reduce_openings must agree with a naive Horner evaluation.  The point of a query index and
// the value of a final polynomial are restated on 128-bit remainders and compared exactly.  A hang ends in SIGALRM.
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <memory>

#include "../../0-kno-vectorx_amd/csrc/stark_proof.h"

namespace sp = stark_proof;
namespace {
#define CHECK(cond)                                                                  \
    do {                                                                             \
        if (!(cond)) {                                                               \
            printf("FAILED %s:%d (%s): %s\n", __FILE__, __LINE__, shape_name, #cond); \
            exit(1);                                                                 \
        }                                                                            \
    } while (0)
char shape_name[160] = "no shape";
constexpr uint64_t COUNTER0 = 1000;  // the first word behind the header (header words are all smaller than this, or the magic)

// every section behind the header, in proof order, as (pointer, words)
template <class W, class F>
void sections(const sp::Proof<W>& p, F f) {
    const sp::Shape& s = *p.s;
    f(p.pub(), s.n_pub), f(p.cap_trace(), s.cap_words);
    if (s.ca) f(p.apub(), 2 * s.auxpub), f(p.cap_aux(), s.cap_words);
    f(p.cap_quot(), s.cap_words);
    f(p.open_local(), 2 * s.c), f(p.open_next(), 2 * s.c), f(p.open_quot(), 2 * sp::NQ);
    for (size_t l = 0; l < s.arities.size(); ++l) f(p.layer_cap(l), s.cap_words);
    f(p.final_poly(), 2 * s.final_len), f(p.nonce(), 1);
    for (size_t k = 0; k < (size_t)s.num_queries; ++k) {
        const sp::Query<W> q = p.query(k);
        f(q.row_t(), s.cm), f(q.sib_t(), 4 * (size_t)s.depth0);
        if (s.ca) f(q.row_a(), s.ca), f(q.sib_a(), 4 * (size_t)s.depth0);
        f(q.row_q(), sp::NQ), f(q.sib_q(), 4 * (size_t)s.depth0);
        for (size_t l = 0; l < s.arities.size(); ++l) f(q.evals(l), 2 * (((size_t)1 << s.arities[l]) - 1)), f(q.sibs(l), 4 * (size_t)s.depth[l]);
    }
}

// the transcript over a proof: every challenge it yields, the query indices last.  `grind` = the prover's call order, which also
// takes the sponge state for the proof of work; `ext` = shared lookup challenges, absorbed instead of drawn
template <class W>
std::vector<uint64_t> run_transcript(const sp::Proof<W>& p, bool grind, const uint64_t* ext) {
    const sp::Shape& s = *p.s;
    std::vector<uint64_t> out;
    auto put = [&out](Fx x) { out.push_back(x.a), out.push_back(x.b); };
    sp::Transcript ch;
    ch.trace(p);
    uint64_t chal[4], alphas[2];
    if (s.ca) {
        ch.lookup_challenges(chal, 4, ext);
        out.insert(out.end(), chal, chal + 4);
        ch.aux(p);
    }
    ch.alphas(alphas);
    out.push_back(alphas[0]), out.push_back(alphas[1]);
    put(ch.zeta(p)), put(ch.alpha(p));
    for (size_t l = 0; l < s.arities.size(); ++l) put(ch.beta(p, l));
    ch.final_poly(p);
    if (grind) {  // the response to a nonce is word 7 of the permuted grind state with the nonce in place
        uint64_t st[12];
        const int n_in = ch.grind_state(st);
        CHECK(n_in >= 0 && n_in < 8);
        st[n_in] = *p.nonce();
        glh::poseidon(st);
        sp::Transcript probe = ch;
        CHECK(probe.pow_ok(*p.nonce(), 8) == ((st[7] >> 56) == 0) && probe.pow_ok(0, 0));
    }
    out.push_back(ch.pow_ok(*p.nonce(), s.pow_bits));
    for (int k = 0; k < s.num_queries; ++k) out.push_back(ch.query_index((size_t)1 << s.LN));
    return out;
}

bool check_shape(const sp::Shape& s) {  // -> the transcript was run too
    const size_t n_hdr = 12 + s.arities.size();
    std::vector<uint64_t> pub(s.n_pub);
    for (size_t i = 0; i < s.n_pub; ++i) pub[i] = COUNTER0 + i;
    sp::Writer w(s, pub.data());
    CHECK(w.words.size() == s.words() && s.words() <= s.bound_words() && s.query_words() * s.num_queries + w.query(0).p - w.pr == (ptrdiff_t)s.words());
    const std::vector<uint64_t> hdr = s.header_words();
    CHECK(hdr.size() == n_hdr && std::equal(hdr.begin(), hdr.end(), w.words.begin()) && hdr[0] == sp::MAGIC && hdr[9] == s.arities.size());
    std::fill(w.words.begin() + n_hdr + s.n_pub, w.words.end(), ~(uint64_t)0);
    uint64_t counter = COUNTER0;
    bool first = true;
    sections<uint64_t>(w, [&](uint64_t* p, size_t n) {
        for (size_t i = 0; i < n; ++i, ++counter)
            if (!first) p[i] = counter;  // (the public inputs were written by the constructor)
        first = false;
    });
    CHECK(counter == COUNTER0 + s.words() - n_hdr);
    for (size_t i = n_hdr; i < s.words(); ++i) CHECK(w.words[i] == COUNTER0 + i - n_hdr);
    // a reader gets the same words back, from a buffer of exactly the proof's length
    const std::vector<uint64_t> exact(w.words);
    sp::View v;
    CHECK(sp::View::parse(exact.data(), exact.size(), s, &v) == nullptr);
    counter = COUNTER0;
    sections<const uint64_t>(v, [&](const uint64_t* p, size_t n) {
        CHECK(p >= exact.data() && p + n <= exact.data() + exact.size());
        for (size_t i = 0; i < n; ++i) CHECK(p[i] == counter++);
    });
    CHECK(counter == COUNTER0 + s.words() - n_hdr);
    // every strict prefix is refused (and one word too many): nothing is handed out
    sp::View none;
    for (size_t len = 0; len < s.words(); ++len) CHECK(sp::View::parse(exact.data(), len, s, &none) != nullptr);
    for (size_t len : {(size_t)0, n_hdr - 1, n_hdr, s.o_cap_trace, s.o_final, s.o_nonce, s.o_queries, s.words() - 1}) {
        const std::unique_ptr<uint64_t[]> cut(new uint64_t[len ? len : 1]);
        std::copy(exact.begin(), exact.begin() + len, cut.get());
        CHECK(sp::View::parse(cut.get(), len, s, &none) != nullptr);
    }
    std::vector<uint64_t> longer(exact);
    longer.push_back(0);
    CHECK(sp::View::parse(longer.data(), longer.size(), s, &none) != nullptr && none.pr == nullptr);
    // the head that is read before the AIR is known
    const uint64_t *ppub = nullptr, *pcap = nullptr;
    size_t pn = 0;
    if (s.cap_h <= 16) CHECK(sp::peek(exact.data(), exact.size(), s.cap_h, &ppub, &pn, &pcap) && ppub == v.pub() && pn == s.n_pub && pcap == v.cap_trace());
    for (size_t len = 0; len < s.o_cap_trace + s.cap_words && s.cap_h <= 4; ++len) CHECK(!sp::peek(exact.data(), len, s.cap_h, &ppub, &pn, &pcap));
    // the transcript: prover's and verifier's call order, challenges drawn and absorbed.  (The host permutation takes 20 us, so
    // only proofs of at most 300 words are hashed: the deepest cap, the empty FRI plan and plans of several layers all occur among them.)
    if (s.words() > 300) return false;
    const uint64_t ext[4] = {11, 22, 33, 44};
    const std::vector<uint64_t> drawn = run_transcript<uint64_t>(w, true, nullptr);
    CHECK(drawn == run_transcript<const uint64_t>(v, false, nullptr));
    if (s.ca) {
        const std::vector<uint64_t> absorbed = run_transcript<uint64_t>(w, true, ext);
        CHECK(absorbed == run_transcript<const uint64_t>(v, false, ext) && absorbed != drawn);
    }
    return true;
}

// ---- reduce_openings against Horner in the extension field, on 128-bit remainders
typedef unsigned __int128 u128;
struct E {
    uint64_t a, b;
};
uint64_t mulmod(uint64_t x, uint64_t y) { return (uint64_t)((u128)x * y % glh::P); }
E emul(E x, E y) { return {(uint64_t)(((u128)mulmod(x.a, y.a) + mulmod(7, mulmod(x.b, y.b))) % glh::P), (uint64_t)(((u128)mulmod(x.a, y.b) + mulmod(x.b, y.a)) % glh::P)}; }
E eadd(E x, E y) { return {(uint64_t)(((u128)x.a + y.a) % glh::P), (uint64_t)(((u128)x.b + y.b) % glh::P)}; }
E horner(const std::vector<E>& coef, E alpha) {
    E acc{0, 0};
    for (size_t j = coef.size(); j-- > 0;) acc = eadd(emul(acc, alpha), coef[j]);
    return acc;
}
void check_reduce() {
    snprintf(shape_name, sizeof shape_name, "reduce_openings");
    uint64_t seed = 0x9e3779b97f4a7c15ULL;
    auto rnd = [&seed]() {
        seed = seed * 6364136223846793005ULL + 1442695040888963407ULL;
        const uint64_t edge[4] = {0, 1, glh::P - 1, glh::P - 2};
        return (seed >> 60) == 0 ? edge[(seed >> 40) & 3] : (seed ^ (seed >> 29)) % glh::P;
    };
    for (size_t c : {1, 2, 7, 40})
        for (size_t nq : {0, 4, 5})
            for (int rep = 0; rep < 20; ++rep) {
                std::vector<uint64_t> local(2 * c), next(2 * c), quot(2 * nq + 1), apow(2 * (c + nq));
                for (auto* v : {&local, &next, &quot})
                    for (uint64_t& x : *v) x = rnd();
                const E alpha{rnd(), rnd()};
                std::vector<E> c0, c1;
                for (size_t j = 0; j < c; ++j) c0.push_back({local[2 * j], local[2 * j + 1]}), c1.push_back({next[2 * j], next[2 * j + 1]});
                for (size_t j = 0; j < nq; ++j) c0.push_back({quot[2 * j], quot[2 * j + 1]});
                const E y0 = horner(c0, alpha), y1 = horner(c1, alpha);
                const sp::Reduced r = sp::reduce_openings(Fx{alpha.a, alpha.b}, local.data(), next.data(), quot.data(), c, nq, apow.data());
                CHECK(r.y0.a == y0.a && r.y0.b == y0.b && r.y1.a == y1.a && r.y1.b == y1.b);
                E p{1, 0};
                for (size_t j = 0; j < c + nq; ++j, p = emul(p, alpha)) {
                    CHECK(apow[2 * j] == p.a && apow[2 * j + 1] == p.b);
                    if (j + 1 == c) CHECK(r.alpha_c.a == emul(p, alpha).a && r.alpha_c.b == emul(p, alpha).b);
                }
                const sp::Reduced r2 = sp::reduce_openings(Fx{alpha.a, alpha.b}, local.data(), next.data(), quot.data(), c, nq);
                CHECK(fx_eq(r2.y0, r.y0) && fx_eq(r2.y1, r.y1) && fx_eq(r2.alpha_c, r.alpha_c));
            }
}

// ---- the point of a query index, 7 w_LN^brev(index), and the final polynomial at a base-field point, restated: w_LN by squaring
// the 2^32-th root of unity 7^((p - 1) / 2^32), the power bit by bit from the index's LOW bit (which weighs 2^(LN - 1) reversed)
uint64_t powmod(uint64_t x, uint64_t e) {
    uint64_t r = 1;
    for (; e; e >>= 1, x = mulmod(x, x))
        if (e & 1) r = mulmod(r, x);
    return r;
}
uint64_t point_restated(uint64_t index, int LN) {
    uint64_t w = powmod(7, (glh::P - 1) >> 32);
    for (int i = 32; i > LN; --i) w = mulmod(w, w);
    uint64_t x = 7;
    for (int b = 0; b < LN; ++b)
        if ((index >> b) & 1) x = mulmod(x, powmod(w, (uint64_t)1 << (LN - 1 - b)));
    return x;
}
void check_query_point_and_final_poly() {
    snprintf(shape_name, sizeof shape_name, "query_point");
    CHECK(sp::brev(0, 0) == 0 && sp::brev(1, 1) == 1 && sp::brev(1, 5) == 16 && sp::brev(0b10110, 5) == 0b01101 && sp::brev(((size_t)1 << 21) - 2, 21) == ((size_t)1 << 20) - 1);
    for (uint64_t i = 0; i < 32; ++i) CHECK(sp::query_point(i, 5) == point_restated(i, 5));
    CHECK(sp::query_point(0, 5) == 7 && sp::query_point(1, 5) == glh::P - 7);  // w^(N / 2) = -1
    uint64_t seed = 0x2545f4914f6cdd1dULL;
    auto rnd = [&seed]() {
        seed = seed * 6364136223846793005ULL + 1442695040888963407ULL;
        return (seed ^ (seed >> 29)) % glh::P;
    };
    const uint64_t N21 = (uint64_t)1 << 21;
    for (uint64_t i : {(uint64_t)0, (uint64_t)1, N21 - 1, N21 - 2, N21 >> 1}) CHECK(sp::query_point(i, 21) == point_restated(i, 21));
    for (int rep = 0; rep < 64; ++rep) {
        const uint64_t i = rnd() % N21, x = sp::query_point(i, 21);
        CHECK(x == point_restated(i, 21) && powmod(mulmod(x, powmod(7, glh::P - 2)), N21) == 1);  // x / 7 lies in the subgroup of order 2^21
    }
    snprintf(shape_name, sizeof shape_name, "final_poly_at");
    for (size_t len : {1, 2, 8})
        for (int rep = 0; rep < 20; ++rep) {
            std::vector<uint64_t> words(2 * len);
            for (uint64_t& w : words) w = rep == 0 ? glh::P - 1 : rnd();
            const uint64_t x = rep == 1 ? 0 : rep == 2 ? glh::P - 1 : rnd();
            std::vector<E> coef;
            for (size_t k = 0; k < len; ++k) coef.push_back({words[2 * k], words[2 * k + 1]});
            const E want = horner(coef, E{x, 0});
            const Fx got = sp::final_poly_at(words.data(), len, x);
            CHECK(got.a == want.a && got.b == want.b);
            if (len == 1) CHECK(got.a == words[0] && got.b == words[1]);
        }
}
}  // namespace

int main() {
    alarm(30);
    size_t n_shapes = 0, n_transcripts = 0, deepest_cap = 0, no_layers = 0, with_layers = 0;  // (the last three: among the shapes whose transcript ran)
    for (int L = 2; L <= 12; ++L)
        for (int r = 1; r <= 3; ++r)
            for (int cap_h : {0, 2, 4, L + r})
                for (int ca : {0, 3})
                    for (int auxpub : {0, 1})
                        for (int arity_bits : {1, 4, 5})
                            for (int final_poly_bits : {0, 5})
                                for (int queries : {1, 3}) {
                                    if (cap_h > L + r) continue;  // (cap 4 above a 2^3 LDE: refused by prover and verifier alike)
                                    vx_stark_config cfg{};
                                    cfg.rate_bits = r, cfg.cap_height = cap_h, cfg.num_queries = queries, cfg.pow_bits = 8 * (queries - 1);
                                    cfg.arity_bits = arity_bits, cfg.final_poly_bits = final_poly_bits;
                                    snprintf(shape_name, sizeof shape_name, "L %d r %d cap %d ca %d auxpub %d arity %d final %d queries %d", L, r, cap_h, ca, auxpub, arity_bits,
                                             final_poly_bits, queries);
                                    CHECK(sp::config_ok(cfg));
                                    const sp::Shape s(/*air id*/ 7 + ca, /*cm*/ 5, ca, /*n_pub*/ (size_t)(L % 4), auxpub, L, cfg);
                                    CHECK(s.depth0 == L + r - cap_h && s.depth.size() == s.arities.size());
                                    for (int d : s.depth) CHECK(d >= 0);
                                    const bool transcript = check_shape(s);
                                    ++n_shapes, n_transcripts += transcript, deepest_cap += transcript && s.depth0 == 0, no_layers += transcript && s.arities.empty(), with_layers += transcript && s.arities.size() > 1;
                                }
    snprintf(shape_name, sizeof shape_name, "the grid");
    CHECK(deepest_cap > 0 && no_layers > 0 && with_layers > 0);
    check_reduce();
    check_query_point_and_final_poly();
    printf("ok %zu %zu\n", n_shapes, n_transcripts);
    return 0;
}
