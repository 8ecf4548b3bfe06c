// The host challengers of 0-kno-vectorx_amd/csrc/glh_poseidon.h and the transcript over them (stark_proof.h), driven on a CPU:
// over random interleavings of observations and challenges the recording challenger yields what the plain one yields, its record
// -- words, (absorbed, value) per challenge, (k, q) per duplex -- obeys the three plan rules of TranscriptAir (air_transcript.cuh)
// and, REPLAYED block by block from the zero state (overwrite the first k rate words, permute, pop q from the end), reproduces
// every challenge; the claimed challenger fed from the record hands the same values back, notes the same absorbed counts, hashes
// nothing, and reports a run that asks for more than was claimed.  Then the whole Transcript over the three challengers on proofs of
// random words: the same lookup challenges, alphas, zeta, alpha, betas, proof-of-work verdict and query indices.  A hang ends in SIGALRM.
#include <unistd.h>

#include <cstdio>
#include <cstdlib>

#include "../../0-kno-vectorx_amd/csrc/stark_proof.h"

namespace sp = stark_proof;
namespace {
#define CHECK(cond)                                                    \
    do {                                                               \
        if (!(cond)) {                                                 \
            printf("FAILED %s:%d (case %d): %s\n", __FILE__, __LINE__, case_no, #cond); \
            exit(1);                                                   \
        }                                                              \
    } while (0)
int case_no = 0;
uint64_t rng_state = 0x9E3779B97F4A7C15ULL;
uint64_t rnd() {
    rng_state ^= rng_state << 13, rng_state ^= rng_state >> 7, rng_state ^= rng_state << 17;
    return rng_state;
}
uint64_t rnd_field() { return rnd() % glh::P; }

// the chain TranscriptAir proves, from a record alone: -> the challenges in drawing order
std::vector<uint64_t> replay(const glh::TranscriptRecord& r) {
    uint64_t st[12] = {0};
    size_t at = 0;
    std::vector<uint64_t> out;
    for (size_t b = 0; b < r.n_blocks(); ++b) {
        const int k = r.plan[2 * b], q = r.plan[2 * b + 1];
        for (int i = 0; i < k; ++i) st[i] = r.words[at + i];
        at += k;
        glh::poseidon(st);
        for (int t = 0; t < q; ++t) out.push_back(st[7 - t]);
    }
    return out;
}

size_t challengers_agree() {
    size_t n_ops = 0;
    for (case_no = 0; case_no < 1500; ++case_no) {
        glh::Challenger plain;
        glh::RecordingChallenger rec;
        std::vector<uint64_t> drawn;
        const int runs = 1 + (int)(rnd() % 8);
        for (int j = 0; j < runs; ++j) {
            const int n_obs = (int)(rnd() % (j == 0 ? 40 : 20)) + (j == 0), n_draw = (int)(rnd() % (case_no % 3 == 0 ? 20 : 4));
            for (int i = 0; i < n_obs; ++i) {
                const uint64_t x = rnd_field();
                plain.observe(x), rec.observe(x);
            }
            for (int i = 0; i < n_draw; ++i) {
                const uint64_t a = plain.challenge(), b = rec.challenge();
                CHECK(a == b);
                drawn.push_back(a);
            }
            n_ops += n_obs + n_draw;
        }
        // the record: counts, monotone absorbed counts, the three rules, and the replay
        size_t sk = 0, sq = 0;
        for (size_t b = 0; b < rec.n_blocks(); ++b) {
            const int k = rec.plan[2 * b], q = rec.plan[2 * b + 1];
            CHECK(k <= 8 && q <= 8);
            CHECK(k > 0 || q > 0);                      // absorb or squeeze
            CHECK(k == 8 || q > 0);                     // a partial absorption squeezes
            if (k == 0) CHECK(b > 0 && rec.plan[2 * b - 1] == 8);  // absorbs nothing: the previous block was squeezed dry
            sk += k, sq += q;
        }
        CHECK(sk + rec.n_in == rec.words.size() && sq == drawn.size() && rec.n_chal() == drawn.size());
        for (size_t j = 0; j < rec.n_chal(); ++j) {
            CHECK(rec.chal[2 * j + 1] == drawn[j] && rec.chal[2 * j] <= rec.words.size());
            CHECK(j == 0 || rec.chal[2 * j] >= rec.chal[2 * j - 2]);
        }
        CHECK(replay(rec) == drawn);
        // the claimed challenger over the same calls
        glh::ClaimedChallenger cl;
        cl.claims = rec.chal.data(), cl.n_claims = rec.n_chal();
        size_t w = 0;
        for (size_t j = 0; j < rec.n_chal(); ++j) {
            while (w < rec.chal[2 * j]) cl.observe(rec.words[w++]);
            CHECK(cl.challenge() == drawn[j]);
        }
        cl.observe(rec.words.data() + w, rec.words.size() - w);
        CHECK(!cl.short_of && cl.next == cl.n_claims && cl.words == rec.words);
        for (size_t j = 0; j < rec.n_chal(); ++j) CHECK(cl.absorbed[j] == rec.chal[2 * j]);
        CHECK(cl.challenge() == 0 && cl.short_of);  // one more than was claimed
    }
    return n_ops;
}

template <class T>
struct Run {
    uint64_t chal[4], alphas[2];
    Fx zeta, alpha;
    std::vector<Fx> betas;
    bool pow;
    std::vector<size_t> index;
    void go(T& ch, const sp::View& v, const uint64_t* ext) {
        const sp::Shape& s = *v.s;
        ch.trace(v);
        if (s.ca) ch.lookup_challenges(chal, 4, ext), ch.aux(v);
        ch.alphas(alphas);
        zeta = ch.zeta(v), alpha = ch.alpha(v);
        for (size_t l = 0; l < s.arities.size(); ++l) betas.push_back(ch.beta(v, l));
        ch.final_poly(v);
        pow = ch.pow_ok(*v.nonce(), s.pow_bits);
        for (int q = 0; q < s.num_queries; ++q) index.push_back(ch.query_index((size_t)1 << s.LN));
    }
};
template <class A, class B>
bool same(const Run<A>& a, const Run<B>& b, bool aux) {
    if (aux && memcmp(a.chal, b.chal, sizeof a.chal)) return false;
    if (memcmp(a.alphas, b.alphas, sizeof a.alphas) || !fx_eq(a.zeta, b.zeta) || !fx_eq(a.alpha, b.alpha) || a.pow != b.pow || a.index != b.index || a.betas.size() != b.betas.size())
        return false;
    for (size_t l = 0; l < a.betas.size(); ++l)
        if (!fx_eq(a.betas[l], b.betas[l])) return false;
    return true;
}

size_t transcripts_agree() {
    size_t n = 0;
    for (case_no = 0; case_no < 60; ++case_no) {
        const vx_stark_config cfg{1 + case_no % 2, case_no % 5, 1 + case_no % 19, case_no % 3, 4, case_no % 6};
        const int L = 5 + case_no % 7;
        const size_t ca = case_no % 3 == 0 ? 0 : 1 + case_no % 9;
        const sp::Shape shape(5, 1 + case_no % 11, ca, case_no % 4, 1, L, cfg);
        std::vector<uint64_t> pub(shape.n_pub + 1);
        for (uint64_t& x : pub) x = rnd_field();
        sp::Writer wr(shape, pub.data());
        for (size_t i = shape.o_pub; i < wr.words.size(); ++i) wr.words[i] = rnd_field();
        sp::View v;
        CHECK(sp::View::parse(wr.words.data(), wr.words.size(), shape, &v) == nullptr);
        const uint64_t ext[4] = {rnd_field(), rnd_field(), rnd_field(), rnd_field()};
        const uint64_t* e = case_no % 2 ? ext : nullptr;
        sp::Transcript plain;
        sp::TranscriptOf<glh::RecordingChallenger> rec;
        Run<sp::Transcript> a;
        Run<sp::TranscriptOf<glh::RecordingChallenger>> b;
        a.go(plain, v, e), b.go(rec, v, e);
        CHECK(same(a, b, ca > 0));
        sp::TranscriptOf<glh::ClaimedChallenger> cl;
        cl.claims = rec.chal.data(), cl.n_claims = rec.n_chal();
        Run<sp::TranscriptOf<glh::ClaimedChallenger>> c;
        c.go(cl, v, e);
        CHECK(same(a, c, ca > 0) && !cl.short_of && cl.next == cl.n_claims && cl.words == rec.words);
        for (size_t j = 0; j < rec.n_chal(); ++j) CHECK(cl.absorbed[j] == rec.chal[2 * j]);
        CHECK(replay(rec).size() == rec.n_chal() && rec.n_in == 0);  // a transcript ends on a challenge: nothing is left in the buffer
        n += rec.n_blocks();
    }
    return n;
}
}  // namespace

int main() {
    alarm(60);
    const size_t ops = challengers_agree(), blocks = transcripts_agree();
    printf("ok %zu %zu\n", ops, blocks);
    return 0;
}
