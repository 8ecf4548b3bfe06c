// Witness and prover of TranscriptAir (air_transcript.cuh): the Fiat-Shamir transcripts of up to 64 inner proofs, one chain each,
// and vx_stark_transcripts_prove, the table alone on its bus with the verifier outside.  The plan of a chain -- which duplex absorbs
// how many words and yields how many challenges -- is never restated here: it is the record of the ONE challenger
// (glh::RecordingChallenger, glh_poseidon.h), run by the ONE transcript (stark_proof.h) inside the verifier's own code.
//   k_transcript_states  a chain is serial (block b needs the output of block b - 1) and there are few chains (one per inner proof,
//                        about 650 permutations for a hash-chain proof): latency-bound.  16 lanes per chain run the cooperative
//                        permutation of the tree builder (poseidon.cuh), as k_leaf_sponge_states does; per block the first k rate
//                        lanes are overwritten from the flat word buffer, the state ENTERING the block and the rate part leaving
//                        it are stored, and the q challenges popped from the end of the output go to the chain's challenge list
//   k_transcript_trace   one lane per block: the blocks are independent once their entering states exist -- the lane writes the
//                        shape columns and walks the 30 rounds (poseidon_air.cuh) over its 32 rows; idle blocks start from zero
// The auxiliary columns are bus_aux.cuh's, from the AIR's own message list: one lane per block, eight helpers.
// Parity: tests/test_gpu_transcript.py compares trace, auxiliary columns, challenges, the table's proof and the group's blob with
// tests/transcript_ref.py and the reference prover.
#include <string.h>

#include "air_transcript.cuh"
#include "bus_aux.cuh"
#include "glh_poseidon.h"
#include "poseidon.cuh"
#include "poseidon_air.cuh"
#include "vx_bus.h"
#include "vx_internal.h"
#include "vx_table_shapes.h"

namespace {
using namespace tsc;

// per block: meta[4 b ..] = chain id, NABS, NCH, k | q << 8 | START << 16;  per chain: chains[4 c ..] = first block, blocks, where its
// words start in `words`, where its challenges start in `chal`
struct TranscriptArgs {
    const uint64_t *words, *meta, *chains;
    size_t n_chains;
    uint64_t *states, *outs, *chal;  // [blocks][12], [blocks][8], one word per challenge
};

__global__ __launch_bounds__(256) void k_transcript_states(TranscriptArgs a) {
    __shared__ uint64_t lds[16 * 12];
    const int l = threadIdx.x & 15, grp = threadIdx.x >> 4;
    const size_t t = blockIdx.x * (size_t)16 + grp;
    const bool live = t < a.n_chains;
    const uint64_t* ch = a.chains + 4 * (live ? t : a.n_chains - 1);  // surplus groups redo the last chain and do not write
    const size_t b0 = ch[0], b1 = b0 + ch[1];
    const uint64_t* w = a.words + ch[2];
    uint64_t* co = a.chal + ch[3];
    uint64_t s = 0;
    for (size_t b = b0; b < b1; ++b) {
        const uint64_t plan = a.meta[4 * b + 3];
        const int k = (int)(plan & 0xff), q = (int)((plan >> 8) & 0xff);
        if (l < k) s = w[l];  // overwrite mode: a word that is not absorbed keeps the previous output (canonical: checked by the host)
        w += k;
        if (live && l < 12) a.states[12 * b + l] = s;
        s = poseidon_permute_coop(s, l, lds + 12 * grp);
        if (live && l < 8) {
            a.outs[8 * b + l] = s;
            if (l >= 8 - q) co[7 - l] = s;  // the challenger pops out[--n_out]
        }
        co += q;
    }
}

__global__ __launch_bounds__(64) void k_transcript_trace(const uint64_t* __restrict__ states, const uint64_t* __restrict__ outs, const uint64_t* __restrict__ meta, size_t n_active,
                                                         size_t n, uint64_t* __restrict__ tr) {
    const size_t b = blockIdx.x * (size_t)64 + threadIdx.x;
    if (b >= n / 32) return;
    uint64_t s[12], shape[COLS - MSG];
#pragma unroll
    for (int i = 0; i < 12; ++i) s[i] = 0;
#pragma unroll
    for (int j = 0; j < COLS - MSG; ++j) shape[j] = 0;
    if (b < n_active) {
        const uint64_t plan = meta[4 * b + 3];
        const int k = (int)(plan & 0xff), q = (int)((plan >> 8) & 0xff);
        const bool start = (plan >> 16) & 1;
#pragma unroll
        for (int i = 0; i < 12; ++i) s[i] = states[12 * b + i];
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            shape[MSG - MSG + i] = s[i], shape[W - MSG + i] = i < k, shape[Q - MSG + i] = i >= 8 - q;
            shape[PREV - MSG + i] = start ? 0 : outs[8 * (b - 1) + i];  // a block that is no START follows a block of its chain
        }
        shape[CHAIN - MSG] = meta[4 * b], shape[ACT - MSG] = 1, shape[START - MSG] = start, shape[NABS - MSG] = meta[4 * b + 1], shape[NCH - MSG] = meta[4 * b + 2];
    }
    poseidon_air_walk(s, tr, n, 32 * b);
#pragma unroll
    for (int i = 0; i < 8; ++i) shape[OUT - MSG + i] = s[i];
    poseidon_air_block_cols(shape, tr, n, MSG, 32 * b);
}

size_t total_blocks(const glh::TranscriptRecord* chains, size_t n_chains) {
    size_t blocks = 0;
    for (size_t c = 0; c < n_chains; ++c) blocks += chains[c].n_blocks();
    return blocks;
}
TranscriptClaim claim_of(const glh::TranscriptRecord& r) { return {r.words.data(), r.words.size(), r.chal.data(), r.n_chal()}; }
}  // namespace

int32_t TranscriptAir::gen_aux(vx_ctx* ctx, const uint64_t* trace, int log_n, const uint64_t* chal, const uint64_t* pub, uint64_t* aux, uint64_t* aux_pub) {
    return bus_gen_aux<TranscriptAir>(ctx, trace, log_n, chal, pub, aux, aux_pub);
}

void vx_transcript_public(const uint64_t digest[4], uint64_t pub[4]) { memcpy(pub + PUB_DIGEST, digest, 32); }

void vx_stark_transcripts_statement(const TranscriptClaim* chains, size_t n, uint64_t digest[4]) {
    std::vector<uint64_t> w{(uint64_t)n};
    for (size_t c = 0; c < n; ++c) w.push_back(chains[c].n_obs), w.push_back(chains[c].n_chal);
    for (size_t c = 0; c < n; ++c) w.insert(w.end(), chains[c].words, chains[c].words + chains[c].n_obs);
    for (size_t c = 0; c < n; ++c) w.insert(w.end(), chains[c].chal, chains[c].chal + 2 * chains[c].n_chal);
    glh::hash_no_pad(w.data(), w.size(), digest);
}

// The witness of TranscriptAir on the device (vx_bus.h).  The words are canonical and every chain has a block (the callers' checks).
int32_t vx_transcript_trace_dev(vx_ctx* ctx, const glh::TranscriptRecord* chains, size_t n_chains, int log_n, uint64_t* trace_d, uint64_t* chal_out) {
    VX_CHECK(n_chains >= 1 && n_chains <= (size_t)MAX_CHAINS, "transcript: %zu chains (1..%d)", n_chains, MAX_CHAINS);
    const size_t blocks = total_blocks(chains, n_chains);
    VX_CHECK(log_n >= 5 && log_n <= 26 && 32 * blocks <= ((size_t)1 << log_n), "transcript: %zu chains of %zu blocks in all do not fit 2^%d rows", n_chains, blocks, log_n);
    const size_t n = (size_t)1 << log_n;
    std::vector<uint64_t> words, meta(4 * blocks), tab(4 * n_chains);
    size_t b = 0, n_chal = 0;
    for (size_t c = 0; c < n_chains; ++c) {
        const glh::TranscriptRecord& r = chains[c];
        tab[4 * c] = b, tab[4 * c + 1] = r.n_blocks(), tab[4 * c + 2] = words.size(), tab[4 * c + 3] = n_chal;
        uint64_t nabs = 0, nch = 0;
        for (size_t j = 0; j < r.n_blocks(); ++j, ++b) {
            const uint64_t k = r.plan[2 * j], q = r.plan[2 * j + 1];
            meta[4 * b] = c, meta[4 * b + 1] = nabs, meta[4 * b + 2] = nch, meta[4 * b + 3] = k | q << 8 | (uint64_t)(j == 0) << 16;
            nabs += k, nch += q;
        }
        words.insert(words.end(), r.words.begin(), r.words.end());
        n_chal += r.n_chal();
    }
    Scratch sc;
    uint64_t *words_d, *meta_d, *tab_d, *states_d, *outs_d, *chal_d;
    sc.add(words_d, words.size()), sc.add(meta_d, meta.size()), sc.add(tab_d, tab.size()), sc.add(states_d, 12 * blocks), sc.add(outs_d, 8 * blocks), sc.add(chal_d, n_chal);
    sc.alloc(ctx);
    sc.up(words_d, words.data(), words.size() * 8), sc.up(meta_d, meta.data(), meta.size() * 8), sc.up(tab_d, tab.data(), tab.size() * 8);
    sc.sync();  // (the three tables are pageable host memory of this frame)
    if (sc.ok()) {
        const TranscriptArgs a{words_d, meta_d, tab_d, n_chains, states_d, outs_d, chal_d};
        hipLaunchKernelGGL(k_transcript_states, dim3((unsigned)((n_chains + 15) / 16)), dim3(256), 0, ctx->stream, a);  // 16 lanes per chain
        sc.launched();
    }
    if (sc.ok()) {
        hipLaunchKernelGGL(k_transcript_trace, dim3((unsigned)((n / 32 + 63) / 64)), dim3(64), 0, ctx->stream, states_d, outs_d, meta_d, blocks, n, trace_d);
        sc.launched();
    }
    if (chal_out && n_chal) sc.down(chal_out, chal_d, n_chal * 8);
    sc.sync();  // the scratch block goes back to the pool with this frame
    return sc.status("transcript");
}

extern "C" {
int32_t vx_transcript_air_trace(vx_ctx* ctx, size_t n_chains, const size_t* n_ops, const uint64_t* ops, const uint64_t* words, size_t n_words, int log_n, vx_buf* trace_out,
                                uint64_t public_out[4], uint64_t* chal_out) {
    if (!ctx || !n_ops || !ops || !words || !trace_out || !public_out || !chal_out) return VX_ERR_ARG;
    VX_CHECK(n_chains >= 1 && n_chains <= (size_t)MAX_CHAINS, "transcript: %zu chains (1..%d)", n_chains, MAX_CHAINS);
    VX_CHECK(log_n >= 5 && log_n <= 26 && trace_out->n >= ((size_t)COLS << log_n), "transcript: the trace buffer holds %zu elements, too few for %d columns of 2^%d rows (5 <= log_n <= 26)",
             trace_out->n, COLS, log_n);
    for (size_t i = 0; i < n_words; ++i) VX_CHECK(words[i] < glh::P, "transcript: observed word %zu is not canonical", i);
    // every chain through the one challenger: its record is the plan, and the blocks it needs are counted before anything is hashed
    std::vector<glh::TranscriptRecord> chains(n_chains);
    const uint64_t* op = ops;
    size_t at = 0, blocks = 0;
    for (size_t c = 0; c < n_chains; ++c, op += n_ops[c - 1]) {
        size_t obs = 0, drawn = 0;
        for (size_t j = 0; j < n_ops[c]; ++j) {
            VX_CHECK(op[j] <= ((uint64_t)1 << 26), "transcript: chain %zu has a run of %llu operations (at most 2^26)", c, (unsigned long long)op[j]);
            if ((j & 1) && op[j]) VX_CHECK(obs > 0, "transcript: the first operation of chain %zu draws from an empty sponge", c);
            (j & 1 ? drawn : obs) += op[j];
        }
        VX_CHECK(obs + drawn > 0, "transcript: chain %zu is empty", c);
        VX_CHECK(obs <= n_words - at, "transcript: the chains observe more than the %zu words handed over", n_words);
        at += obs, blocks += (obs + 7) / 8 + (drawn + 7) / 8 + n_ops[c];  // an upper bound of its duplexes
    }
    VX_CHECK(at == n_words, "transcript: the chains observe %zu words, %zu were handed over", at, n_words);
    VX_CHECK(blocks <= ((size_t)1 << 24), "transcript: the chains do not fit 2^%d rows", log_n);
    op = ops, at = 0;
    for (size_t c = 0; c < n_chains; ++c, op += n_ops[c - 1]) {
        glh::RecordingChallenger ch;
        for (size_t j = 0; j < n_ops[c]; ++j) {
            if (j & 1) {
                for (uint64_t i = 0; i < op[j]; ++i) ch.challenge();
            } else {
                ch.observe(words + at, op[j]), at += op[j];
            }
        }
        VX_CHECK(ch.n_in == 0, "transcript: chain %zu ends on %d observed words that no duplex absorbs (the challenger duplexes on a full buffer or on a challenge)", c, ch.n_in);
        chains[c] = static_cast<const glh::TranscriptRecord&>(ch);
    }
    VX_TRY(vx_transcript_trace_dev(ctx, chains.data(), n_chains, log_n, trace_out->d, chal_out));
    // the claims: the words, and every challenge as (absorbed, the value the DEVICE drew)
    std::vector<TranscriptClaim> claims;
    size_t k = 0;
    for (glh::TranscriptRecord& r : chains) {
        for (size_t j = 0; j < r.n_chal(); ++j) r.chal[2 * j + 1] = chal_out[k++];
        claims.push_back(claim_of(r));
    }
    uint64_t digest[4];
    vx_stark_transcripts_statement(claims.data(), n_chains, digest);
    vx_transcript_public(digest, public_out);
    return VX_OK;
}

int32_t vx_stark_transcripts_proof_bound(const vx_stark_config* cfg, const uint64_t* const* proofs, const size_t* lens, size_t n, const uint64_t* const* ext_chals, size_t* n_words) {
    if (!cfg || !proofs || !lens || !n_words || n < 1 || n > (size_t)MAX_CHAINS) return VX_ERR_ARG;
    size_t blocks = 0, request = 1;
    for (size_t i = 0; i < n; ++i) {
        glh::TranscriptRecord r;  // the plan depends on the head alone: no query record is read for a bound
        size_t head = 0;
        if (!proofs[i] || vx_stark_proof_head_words(cfg, proofs[i], lens[i], &head) != VX_OK || lens[i] < head) return VX_ERR_ARG;
        if (vx_stark_transcript_record(cfg, proofs[i], head, ext_chals ? ext_chals[i] : nullptr, &r, nullptr, 0) != VX_OK) return VX_ERR_ARG;
        blocks += r.n_blocks(), request += 2 + r.chal.size();
    }
    const int log_n = transcript_log_n(blocks, *cfg);
    if (log_n > 26) return VX_ERR_ARG;
    size_t w = 0;
    const int32_t rc = vx_stark_proof_bound(VX_AIR_TRANSCRIPT, cfg, log_n, &w);
    if (rc != VX_OK) return rc;
    *n_words = 1 + request + 1 + w;
    return VX_OK;
}

int32_t vx_stark_transcripts_prove(vx_ctx* ctx, const vx_stark_config* cfg, const uint64_t* const* proofs, const size_t* lens, size_t n, const uint64_t* const* ext_chals,
                                   uint64_t* blob_out, size_t blob_cap, size_t* blob_len) {
    if (!ctx || !cfg || !proofs || !lens || !blob_len) return VX_ERR_ARG;
    VX_CHECK(n >= 1 && n <= (size_t)MAX_CHAINS, "stark transcripts: %zu proofs (1..%d)", n, MAX_CHAINS);
    // ---- every inner proof verified natively, by the verifier's own code over the recording challenger: its record is the chain
    std::vector<glh::TranscriptRecord> chains(n);
    for (size_t i = 0; i < n; ++i) {
        VX_CHECK(proofs[i], "stark transcripts: proof %zu is missing", i);
        char err[256] = "";
        const int32_t vrc = vx_stark_transcript_record(cfg, proofs[i], lens[i], ext_chals ? ext_chals[i] : nullptr, &chains[i], err, sizeof err);
        if (vrc != VX_OK) return vx_fail(ctx, vrc, "stark transcripts: proof %zu: %s", i, err[0] ? err : "the proof or the configuration is not acceptable");
    }
    const size_t blocks = total_blocks(chains.data(), n);
    const int log_n = transcript_log_n(blocks, *cfg);
    VX_CHECK(log_n <= 26, "stark transcripts: %zu blocks need more than 2^26 rows", blocks);
    std::vector<TranscriptClaim> claims;
    std::vector<uint64_t> request{(uint64_t)n};
    for (const glh::TranscriptRecord& r : chains) {
        claims.push_back(claim_of(r));
        request.push_back(r.words.size()), request.push_back(r.n_chal());
        request.insert(request.end(), r.chal.begin(), r.chal.end());
    }
    uint64_t stmt[4];
    vx_stark_transcripts_statement(claims.data(), n, stmt);
    TableGroup g(ctx, cfg, "stark transcripts");
    const int tab = g.add({"transcript", VX_AIR_TRANSCRIPT, log_n, COLS, PUB, 0, [&](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
                               VX_TRY(vx_transcript_trace_dev(c, chains.data(), n, log_n, trace->d, nullptr));
                               vx_transcript_public(stmt, pub);
                               return (int32_t)VX_OK;
                           }});
    VX_TRY(g.prove(tab));
    const TableJob* jobs[1] = {&g.job[tab]};
    return pack_blob(ctx, "stark transcripts", VX_STRN_MAGIC, request.data(), request.size(), jobs, 1, blob_out, blob_cap, blob_len);
}
}  // extern "C"
