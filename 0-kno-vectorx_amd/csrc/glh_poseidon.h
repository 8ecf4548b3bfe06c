// The ONE host-side Poseidon-Goldilocks permutation and duplex challenger (plonky2 v0.2.0 hash/poseidon.rs,
// iop/challenger.rs: width 12, rate 8, overwrite-mode duplexing) -- used by the prover's transcript (vx_stark.hip) and by
// the host verifiers (vx_verify.hip: transcript, Merkle paths, leaf hashing).  Host code only; the device permutation
// is poseidon.cuh.  Round constants and the circulant MDS row come from the generated poseidon_constants.h.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "glh.h"
#include "poseidon_constants.h"

namespace glh {
inline void poseidon(uint64_t* s) {
    static const uint64_t RC[360] = VX_POSEIDON_RC_INIT;
    static const uint64_t MDS[12] = VX_POSEIDON_MDS_CIRC_INIT;
    for (int r = 0; r < 30; ++r) {
        for (int i = 0; i < 12; ++i) s[i] = add(s[i], RC[12 * r + i]);
        const int nsb = (r < 4 || r >= 26) ? 12 : 1;  // 4 + 4 full rounds around 22 partial ones
        for (int i = 0; i < nsb; ++i) {
            const uint64_t x = s[i], x2 = mul(x, x), x3 = mul(x2, x), x4 = mul(x2, x2);
            s[i] = mul(x3, x4);
        }
        uint64_t o[12];
        for (int row = 0; row < 12; ++row) {
            unsigned __int128 acc = 0;
            for (int i = 0; i < 12; ++i) acc += (unsigned __int128)s[(i + row) % 12] * MDS[i];
            if (row == 0) acc += (unsigned __int128)s[0] * VX_POSEIDON_MDS_DIAG0;
            o[row] = reduce128(acc);
        }
        memcpy(s, o, sizeof o);
    }
}
// hash_n_to_hash_no_pad (hash/hashing.rs): the sponge absorbs 8 words per permutation by overwriting the rate part
inline void hash_no_pad(const uint64_t* in, size_t len, uint64_t out4[4]) {
    uint64_t s[12] = {0};
    for (size_t off = 0; off < len; off += 8) {
        memcpy(s, in + off, (len - off < 8 ? len - off : 8) * 8);
        poseidon(s);
    }
    memcpy(out4, s, 32);
}
// compress / two_to_one: the parent of two digests
inline void two_to_one(const uint64_t l[4], const uint64_t r[4], uint64_t out4[4]) {
    uint64_t s[12] = {0};
    memcpy(s, l, 32), memcpy(s + 4, r, 32);
    poseidon(s);
    memcpy(out4, s, 32);
}
// the digest of a Merkle leaf (hash_or_noop): a row of at most 4 words is its own digest, zero-padded
inline void hash_or_noop(const uint64_t* in, size_t len, uint64_t out4[4]) {
    if (len > 4) return hash_no_pad(in, len, out4);
    memset(out4, 0, 32);
    memcpy(out4, in, len * 8);
}
// verify_merkle_proof_to_cap: leaf `idx` under `n_sib` siblings (4 words each) must arrive at its entry of the cap
inline bool merkle_path_ok(const uint64_t* leaf, size_t leaf_len, size_t idx, const uint64_t* sib, size_t n_sib, const uint64_t* cap) {
    uint64_t cur[4];
    hash_or_noop(leaf, leaf_len, cur);
    for (size_t k = 0; k < n_sib; ++k, idx >>= 1) {
        if (idx & 1) two_to_one(sib + 4 * k, cur, cur);
        else two_to_one(cur, sib + 4 * k, cur);
    }
    return memcmp(cur, cap + 4 * idx, 32) == 0;
}
// The duplex challenger, stated once over a recorder R: what it is told about every duplex, absorbed word and drawn challenge.
// Challenger records nothing; RecordingChallenger (the prover of TranscriptAir, air_transcript.cuh) keeps the chain's witness.
struct NoRecord {
    void duplexed(int) {}
    void observed(uint64_t) {}
    void drawn(uint64_t) {}
};
template <class R>
struct ChallengerOf : R {
    uint64_t st[12] = {0}, in[8], out[8];
    int n_in = 0, n_out = 0;
    void duplex() {
        R::duplexed(n_in);
        for (int i = 0; i < n_in; ++i) st[i] = in[i];
        n_in = 0;
        poseidon(st);
        memcpy(out, st, sizeof out);
        n_out = 8;
    }
    void observe(uint64_t x) {
        R::observed(x);
        n_out = 0;
        in[n_in++] = x;
        if (n_in == 8) duplex();
    }
    void observe(const uint64_t* x, size_t n) {
        for (size_t i = 0; i < n; ++i) observe(x[i]);
    }
    uint64_t challenge() {
        if (n_in > 0 || n_out == 0) duplex();
        R::drawn(out[n_out - 1]);
        return out[--n_out];
    }
};
using Challenger = ChallengerOf<NoRecord>;
// What a transcript did, as TranscriptAir's chain: the absorbed words in order, every challenge as (words absorbed when it was drawn,
// value), and per duplex (k, q) = words absorbed by it, challenges popped from its output.
struct TranscriptRecord {
    std::vector<uint64_t> words, chal;
    std::vector<uint8_t> plan;
    void duplexed(int k) { plan.push_back((uint8_t)k), plan.push_back(0); }
    void observed(uint64_t x) { words.push_back(x); }
    void drawn(uint64_t v) { ++plan.back(), chal.push_back(words.size()), chal.push_back(v); }
    size_t n_chal() const { return chal.size() / 2; }
    size_t n_blocks() const { return plan.size() / 2; }
};
using RecordingChallenger = ChallengerOf<TranscriptRecord>;
// The verifier's side of a transcript somebody else proves: it hashes NOTHING.  observe appends to the words it will send,
// challenge returns the next claimed value -- claims: n_claims pairs (absorbed, value) -- and notes how many words were absorbed
// by then.  A run that asks for more challenges than are claimed is answered with zeros and `short_of` is set: the caller checks
// next == n_claims && !short_of before it believes anything the run concluded.
struct ClaimedChallenger {
    const uint64_t* claims = nullptr;
    size_t n_claims = 0, next = 0;
    bool short_of = false;
    std::vector<uint64_t> words, absorbed;
    void observe(uint64_t x) { words.push_back(x); }
    void observe(const uint64_t* x, size_t n) { words.insert(words.end(), x, x + n); }
    uint64_t challenge() {
        absorbed.push_back(words.size());
        if (next >= n_claims) return short_of = true, 0;
        return claims[2 * next++ + 1];
    }
};
}  // namespace glh
