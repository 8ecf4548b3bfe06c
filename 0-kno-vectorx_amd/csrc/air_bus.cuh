// The logUp bus every lookup AIR shares: the tags, the denominator of a message, and the slot order of every message kind.
// A message is (t0, t1, t2, t3, tag); the prover's helper columns hold m / D with
//     D = beta + t0 + gamma t1 + gamma^2 t2 + gamma^3 t3 + gamma^4 tag        (beta, gamma: extension-field challenges)
// and the tables' published totals cancel when every message sent is received.  What a slot MEANS is a contract between the
// table that sends a kind and the table that receives it, so each kind is one named function here and both sides -- in `eval`
// (X = X2<F>: device FpN<R>, host Fx, CountF) and in the witness kernel (X = gl2; X2<Fp> in bus_aux.cuh, which reads a table's
// whole message list from the AIR: air.cuh "the bus of a table ...") -- call that name.  The oracle (oracle/*.py: one
// fp(tag, tuple)) restates tags and slot orders independently on purpose.
#pragma once
#include <type_traits>

#include "gl.cuh"

namespace bus {
enum Tag : uint64_t { TAG_T1 = 0, TAG_T2 = 1, TAG_BYTE = 2, TAG_WORD = 3, TAG_R16 = 4, TAG_KEY = 5, TAG_EDMSG = 6, TAG_EDH = 7, TAG_OPEN = 8, TAG_ROW = 9, TAG_FRI = 10, TAG_ROOT = 11, TAG_OBS = 12, TAG_CHAL = 13, TAG_FIN = 14 };

// a slot known at compile time: 0 leaves its term out, 1 adds the bare power of gamma, so a kind that does not use a slot
// (or whose tag is 0 or 1) costs what the hand-written sum cost
template <uint64_t N>
struct K {};
using None = K<0>;

template <class X>  // X2<F> or gl2; S = its base field (F or uint64_t)
struct Bus {
    using S = decltype(X::a);
    X beta, gamma, g2, g3, g4;
    VX_HD Bus(const S& c0, const S& c1, const S& c2, const S& c3) : beta{c0, c1}, gamma{c2, c3}, g2(gamma * gamma), g3(g2 * gamma), g4(g2 * g2) {}

    VX_HD static S lit(uint64_t n) {
        if constexpr (std::is_same<S, uint64_t>::value) return n;
        else return S::from(n);
    }
    // 2 t + N for a slot that packs a small compile-time part under a field value (a tree id is below 2^32: no reduction needed)
    template <uint64_t N>
    VX_HD static S twice_plus(const S& t, K<N>) {
        if constexpr (std::is_same<S, uint64_t>::value) return 2 * t + N;
        else if constexpr (N == 0) return t + t;
        else return t + t + lit(N);
    }
    VX_HD static X plus(const X& acc, const S& t) { return acc + t; }
    VX_HD static X plus(const X& acc, None) { return acc; }
    VX_HD static X term(const X& acc, const X& g, const S& t) { return acc + g * t; }
    template <uint64_t N>
    VX_HD static X term(const X& acc, const X& g, K<N>) {
        if constexpr (N == 0) return acc;
        else if constexpr (N == 1) return acc + g;
        else return acc + g * lit(N);
    }
    // The denominator, written once.  A slot is a field value or a K<N>.  `base` is beta, or beta plus the slots a caller has
    // hoisted out of a loop (a *_base below); those slots are then None.  The tag is a field value where EdAir and Sha512Air
    // mix tags with row selectors.
    template <class T0, class T1, class T2, class T3, class TG>
    VX_HD X denom(const X& base, const T0& t0, const T1& t1, const T2& t2, const T3& t3, const TG& tag) const {
        return term(term(term(term(plus(base, t0), gamma, t1), g2, t2), g3, t3), g4, tag);
    }

    // ---- the message kinds: sender -> receiver ----
    // table 1, a row (a, b, a ^ b) of an XOR table: BlakeAir's G functions and byte range checks (b = None) -> its own periodic table; LookupAir alike
    template <class B>
    VX_HD X xor_row(const S& a, const B& b, const S& c) const { return denom(beta, a, b, c, None{}, K<TAG_T1>{}); }
    // table 2, a row (a, b, (a ^ b) & 127, (a ^ b) >> 7): BlakeAir -> its own periodic table
    VX_HD X t2_base() const { return denom(beta, None{}, None{}, None{}, None{}, K<TAG_T2>{}); }
    VX_HD X t2_row(const X& t2_base_, const S& a, const S& b, const S& lo7, const S& hi1) const { return denom(t2_base_, a, b, lo7, hi1, None{}); }
    // a header byte (leaf, position, byte, tree): BlakeAir -> ShaTreeAir (roots; tree 0 state, 1 data) and EpochEndAir (leaf None, tree K<1>)
    template <class L, class T>
    VX_HD X byte_base(const L& leaf, const T& tree) const { return denom(beta, leaf, None{}, None{}, tree, K<TAG_BYTE>{}); }
    VX_HD X byte(const X& byte_base_, const S& position, const S& byte_) const { return denom(byte_base_, None{}, position, byte_, None{}, None{}); }
    // a digest or message word (tree, node, j, word): ShaTreeAir's PAD blocks -> its parents' DATA blocks
    VX_HD X word_base() const { return denom(beta, None{}, None{}, None{}, None{}, K<TAG_WORD>{}); }
    VX_HD X word(const X& word_base_, const S& tree, const S& node, const S& j, const S& w) const { return denom(word_base_, tree, node, j, w, None{}); }
    // a 16-bit range value (v): EdAir's cells -> its own periodic table
    VX_HD X r16_base() const { return denom(beta, None{}, None{}, None{}, None{}, K<TAG_R16>{}); }
    VX_HD X r16(const X& r16_base_, const S& v) const { return denom(r16_base_, v, None{}, None{}, None{}, None{}); }
    // a key quarter (4 index + j, l0 + 2^16 l1, l2 + 2^16 l3) of 16-bit limbs: ShaChainAir -> EdAir, EpochEndAir -> ShaChainAir
    VX_HD X key(const S& quarter, const S& lo, const S& hi) const { return denom(beta, quarter, lo, hi, None{}, K<TAG_KEY>{}); }
    // a part of R || A (4 slot + part, three / three / two 16-bit limbs packed little-endian): EdAir -> Sha512Air
    VX_HD X ed_msg(const S& part, const S& u1, const S& u2, const S& u3) const { return denom(beta, part, u1, u2, u3, K<TAG_EDMSG>{}); }
    // a part of the digest (8 slot + part, three 32-bit halves): Sha512Air -> EdAir
    VX_HD X ed_digest(const S& part, const S& h0, const S& h1, const S& h2) const { return denom(beta, part, h0, h1, h2, K<TAG_EDH>{}); }
    // half of an opened leaf digest (leaf index, d[2 half], d[2 half + 1], half): MerkleOpenAir -> whoever holds the openings (the
    // verifier of vx_merkle_openings_verify; LeafSpongeAir, which hashes the opened rows to these digests)
    template <class H>
    VX_HD X open(const S& index, const S& da, const S& db, const H& half) const { return denom(beta, index, da, db, half, K<TAG_OPEN>{}); }
    // ... of one of several trees (leaf index, d[2 half], d[2 half + 1], half + 2 tree): tree 0 is the very message open() builds.
    // MerkleOpenSetAir -> LeafSpongeSetAir
    template <uint64_t H>
    VX_HD X open_of(const S& tree, const S& index, const S& da, const S& db, K<H> half) const { return denom(beta, index, da, db, twice_plus(tree, half), K<TAG_OPEN>{}); }
    // half of the root a path of one of several trees ended in, with that tree's depth (2 tree + half, r[2 half], r[2 half + 1],
    // depth): MerkleOpenSetAir -> whoever knows the trees (the verifier of vx_fri_queries_verify)
    template <uint64_t H>
    VX_HD X root(const S& tree, const S& ra, const S& rb, K<H> half, const S& depth) const { return denom(beta, twice_plus(tree, half), ra, rb, depth, K<TAG_ROOT>{}); }
    // one word of an opened leaf row (leaf index, position in the row, word): LeafSpongeAir -> whoever holds the rows (the verifier)
    VX_HD X row(const S& index, const S& position, const S& word) const { return denom(beta, index, position, word, None{}, K<TAG_ROW>{}); }
    // ... of one of several trees (leaf index, position in the row, word, tree): tree 0 is the very message row() builds, so a
    // one-layer FRI with TREE0 = 0 is already receivable from LeafSpongeAir (that pairing is not built).  LeafSpongeSetAir sends
    // them for every tree -> FriFoldAir, which receives the leaves of FRI layer l under tree TREE0 + l (vx_fri_queries_prove), or
    // the verifier (vx_fri_fold_verify).  FriCombineAir RECEIVES the opened commitment-tree rows one word per message under tree
    // TREE0 + 0 main / 1 auxiliary / 2 quotient (TREE0 = 8 in its entry points); today the verifier sends them
    // (vx_fri_combine_verify, vx_fri_combine_fold_verify)
    template <class T>
    VX_HD X row_of(const T& tree, const S& index, const S& position, const S& word) const { return denom(beta, index, position, word, tree, K<TAG_ROW>{}); }
    // an end of a query's fold chain (query index, value.a, value.b, end): end 0 = (index, ev_0) entering the chain, whoever
    // computes the FRI combination (FriCombineAir in vx_fri_combine_fold_prove, else the verifier) -> FriFoldAir, or FriCombineAir
    // -> the verifier (vx_fri_combine_verify); end 1 = (index, ev_NL) leaving it, FriFoldAir -> whoever
    // evaluates the final polynomial (the verifier)
    template <class E>
    VX_HD X fri(const S& index, const S& va, const S& vb, const E& end) const { return denom(beta, index, va, vb, end, K<TAG_FRI>{}); }
    // a word a Fiat-Shamir transcript absorbs (chain, position among the chain's absorbed words, word): whoever holds the proof (the
    // verifier of vx_stark_transcripts_verify) -> TranscriptAir
    VX_HD X obs(const S& chain, const S& position, const S& word) const { return denom(beta, chain, position, word, None{}, K<TAG_OBS>{}); }
    // a challenge a transcript yields (chain, ordinal among the chain's challenges, words absorbed when it was drawn, value):
    // TranscriptAir -> whoever uses the challenges (the verifier).  `absorbed` binds WHEN: without it the absorptions could be regrouped
    VX_HD X chal(const S& chain, const S& ordinal, const S& absorbed, const S& word) const { return denom(beta, chain, ordinal, absorbed, word, K<TAG_CHAL>{}); }
    // a coefficient of an inner proof's final polynomial (k, c_k.a, c_k.b): whoever holds the proof head (the verifier of
    // fri_exits_verify, once per query) -> FriExitAir, which evaluates the polynomial at every query's point
    VX_HD X fin(const S& k, const S& ca, const S& cb) const { return denom(beta, k, ca, cb, None{}, K<TAG_FIN>{}); }
};
}  // namespace bus
