// HeaderRangeCircuit (circuits/header_range.rs): vx_header_range_prove(_ex) -- the statement natively, then its tables on one
// logUp bus (vx_bus.h), each proven on a context of its own -- the proof bounds, and vx_header_range_merge (host only) for the
// blobs of a proof whose tables were proven by several processes.  The verifier is vx_header_range_verify in vx_verify.hip.
#include <string.h>

#include "vx_bus.h"
#include "vx_table_shapes.h"

static const uint64_t VX_HR_MAGIC = VX_HR_BLOB_MAGIC;  // "HRRANGE6" (include/vx.h)
// magic, max_headers, trusted, target, out96 (12), proof lengths: hash chain, authority-set commitment, Merkle, Ed25519, SHA-512; the precommit's round
static const size_t VX_HR_HDR = VX_HR_BLOB_FIXED_WORDS + 1;  // one segment

// Map segments: contiguous runs of headers with (nearly) equal numbers of Blake2b compressions.  bounds[s] .. bounds[s + 1]
static void hr_segments(const uint32_t* sizes, size_t n, uint32_t S, std::vector<size_t>& bounds, std::vector<size_t>& chunks) {
    size_t total = 0;
    for (size_t i = 0; i < n; ++i) total += (sizes[i] + 127) / 128;
    bounds.assign(1, 0), chunks.clear();
    size_t acc = 0, seg = 0;
    for (size_t i = 0; i < n; ++i) {
        acc += (sizes[i] + 127) / 128, seg += (sizes[i] + 127) / 128;
        const size_t s = bounds.size();  // the segment being filled is s - 1
        const size_t left_h = n - 1 - i, left_s = S - s;  // headers / segments still to come
        if (s < S && (acc * S >= s * total || left_h == left_s) && left_h >= left_s) bounds.push_back(i + 1), chunks.push_back(seg), seg = 0;
    }
    bounds.push_back(n), chunks.push_back(seg);
}

static int32_t hr_prove(vx_ctx* ctx, const vx_buf* headers, size_t stride, const uint32_t* sizes, size_t n_fetched, uint32_t max_headers, uint32_t trusted_block,
                        const uint8_t trusted_hash[32], uint32_t target_block, const vx_justification* just, const vx_stark_config* cfg, uint32_t S, uint32_t shard,
                        uint32_t n_shards, const vx_hr_exchange* xch, uint8_t out96[96], uint64_t* proof_out, size_t proof_cap, size_t* proof_len) {
    if (!ctx || !cfg || !proof_len || !out96) return VX_ERR_ARG;
    const int tree_id = tree_air_id(max_headers);
    VX_CHECK(tree_id, "header_range: max_headers %u has no Merkle AIR (16, 256 or 512)", max_headers);
    VX_CHECK(!just || (just->num_authorities >= 1 && just->num_authorities <= 512), "header_range: %u authorities (the EdDSA table holds 512)", just ? just->num_authorities : 0);
    VX_CHECK(S >= 1 && S <= VX_HR_MAX_SEGMENTS && S <= n_fetched, "header_range: %u map segments for %zu headers (1 .. %d, at most one per header)", S, n_fetched, (int)VX_HR_MAX_SEGMENTS);
    VX_CHECK(n_shards >= 1 && shard < n_shards && (n_shards == 1 || (xch && xch->fn)), "header_range: shard %u of %u (an exchange function goes with more than one shard)", shard, n_shards);
    VX_CHECK(cfg->cap_height >= 0 && cfg->cap_height <= 8, "header_range: cap_height %d", cfg->cap_height);
    // 1. statement + public outputs (map/reduce chain rules, Merkle roots)
    VX_TRY(vx_verify_subchain(ctx, headers, stride, sizes, n_fetched, max_headers, trusted_block, trusted_hash, target_block, out96));
    const size_t HDR = VX_HR_BLOB_FIXED_WORDS + S;
    const int tl = tree_log_n(max_headers);
    // 2. the tables, all on ONE logUp bus under shared lookup challenges (one TableGroup, vx_bus.h), in bus order:
    //    0 .. S-1  BlakeChainAir   map segment s: every compression of its headers; sends state-root and data-root bytes
    //    S         ShaTreeAir      the two SHA-256 Merkle trees over exactly those roots (subchain_verification.rs:213-220, 268-274)
    //   with a justification (header_range.rs:49-54 -> justification.rs:195-257):
    //    S+1       ShaChainAir     the authority-set commitment (justification.rs:127-162); sends the keys of the signed authorities
    //    S+2       EdAir           [S]B = R + [h]A for every signed authority (:229-243); receives the keys, exchanges R || A / H with
    //    S+3       Sha512Air       H = SHA-512(R || A || precommit)
    //   table t is proven here when t mod n_shards == shard
    auto mine = [&](int t) { return (uint32_t)t % n_shards == shard; };
    std::vector<size_t> bounds, seg_chunks;
    hr_segments(sizes, n_fetched, S, bounds, seg_chunks);
    std::vector<uint8_t> digests;  // the hash every segment starts from: the Blake2b-256 digest of the header before it
    std::vector<uint32_t> numbers(n_fetched);
    std::vector<uint8_t> modes(n_fetched), oks(n_fetched), parents(32 * n_fetched), sroots(32 * n_fetched), droots(32 * n_fetched);
    // the target header is justified by > 2/3 of the committed authority set: every rule natively first (error behaviour of
    // the reference's hint, justification.rs:29-83) -- on the commitment table's thread, or here when that table is another shard's
    auto pre = [=](vx_ctx* c) {
        return vx_verify_simple_justification(c, target_block, out96, just->authority_set_id, just->authority_set_hash, just->precommit, just->pubkeys, just->signatures,
                                              just->validator_signed, just->num_authorities, just->max_authorities);
    };
    // From here on the other shards of a sharded proof count on this one at the exchange: whichever way this function is left, the
    // group fails the local tables that were never started (they arrive as failure markers) before it goes.
    TableGroup g(ctx, cfg, "header_range");
    g.g.shard(n_shards > 1 ? xch : nullptr, (size_t)4 << cfg->cap_height);
    for (int s = 0; s < (int)S; ++s) {
        const size_t a = bounds[s], b = bounds[s + 1];
        const int log_n = blake_log_n(seg_chunks[s]);
        g.add({"hash-chain segment", VX_AIR_BLAKE_CHAIN, log_n, VX_BLAKE_AIR_COLS, 20, /*consume_trace=*/1,
               [&, a, b, log_n](vx_ctx* c, vx_buf* trace, uint64_t* pub) {
                   vx_buf view{headers->d + a * stride / 8, headers->n - a * stride / 8};
                   VX_TRY(vx_blake_chain_trace(c, &view, stride, sizes + a, b - a, a ? digests.data() + 32 * (a - 1) : trusted_hash, trusted_block + 1 + (uint32_t)a, max_headers, (uint32_t)a,
                                               0, log_n, trace, pub, nullptr));
                   if (b == n_fetched) {
                       uint8_t tgt[32];
                       for (int q = 0; q < 8; ++q) {
                           uint32_t l = (uint32_t)pub[8 + q];
                           memcpy(tgt + 4 * q, &l, 4);
                       }
                       if (memcmp(tgt, out96, 32) != 0) return vx_fail(c, VX_ERR_STATEMENT, "header_range: chain digest differs from the subchain target hash");
                   }
                   return (int32_t)VX_OK;
               }},
              0, mine(s));
    }
    g.add({"Merkle", tree_id, tl, VX_SHA_TREE_AIR_COLS, 17, /*consume_trace=*/0,
           [&](vx_ctx* c, vx_buf* tt, uint64_t* tpub) {
               VX_TRY(vx_sha_tree_trace_dev(c, sroots.data(), droots.data(), n_fetched, tl - 8, tt->d, tpub));
               uint8_t roots[64];
               for (int q = 0; q < 16; ++q)
                   for (int b = 0; b < 4; ++b) roots[4 * q + b] = (uint8_t)(tpub[q] >> (24 - 8 * b));
               if (memcmp(roots, out96 + 32, 64) != 0) return vx_fail(c, VX_ERR_STATEMENT, "header_range: Merkle AIR roots differ from the subchain roots");
               return (int32_t)VX_OK;
           }},
          0, mine((int)S));
    if (just) vx_justification_add(g, just, pre, 0, (mine((int)S + 1) ? 1u : 0) | (mine((int)S + 2) ? 2u : 0) | (mine((int)S + 3) ? 4u : 0));
    if (S > 1) {
        digests.resize(32 * n_fetched);
        VX_TRY(vx_blake2b_256_batch(ctx, headers, stride, sizes, n_fetched, digests.data()));
    }
    // the leaves of the two Merkle trees: decode_header on the GPU (all four compact modes)
    if (mine((int)S)) VX_TRY(vx_decode_header_batch(ctx, headers, stride, sizes, n_fetched, numbers.data(), modes.data(), oks.data(), parents.data(), sroots.data(), droots.data()));
    if (just && !mine((int)S + 1)) VX_TRY(pre(ctx));
    // the first local segment runs on `ctx` from this thread, every other local table on the chain of side contexts; failures are
    // reported in the order: the justification's tables (its own rules name the error first), the Merkle table, the segments
    int main_seg = -1;
    for (int t = 0; t < (int)S && main_seg < 0; ++t)
        if (mine(t)) main_seg = t;
    std::vector<int> report;
    for (int t = (int)S + 1; t < g.g.n; ++t) report.push_back(t);
    report.push_back((int)S);
    for (int s = 0; s < (int)S; ++s) report.push_back(s);
    VX_TRY(g.prove(main_seg, report));
    const TableJob *seg = g.job, &tree = g.job[S], *jt = &g.job[S + 1];  // (jt only with a justification)
    size_t total = HDR + tree.len + (just ? jt[0].len + jt[1].len + jt[2].len : 0);
    for (int s = 0; s < (int)S; ++s) total += seg[s].len;
    *proof_len = total;
    if (!proof_out || proof_cap < total) return vx_fail(ctx, VX_ERR_BUFSZ, "header_range: proof needs %zu words, buffer has %zu", total, proof_cap);
    size_t off = HDR;
    for (int s = 0; s < (int)S; ++s) memcpy(proof_out + off, seg[s].proof.data(), seg[s].len * 8), off += seg[s].len;
    const TableJob* order[4] = {just ? &jt[0] : nullptr, &tree, just ? &jt[1] : nullptr, just ? &jt[2] : nullptr};  // commitment, Merkle, Ed25519, SHA-512
    for (int q = 0; q < 4; ++q)
        if (order[q]) memcpy(proof_out + off, order[q]->proof.data(), order[q]->len * 8), off += order[q]->len;
    proof_out[0] = VX_HR_MAGIC;
    proof_out[1] = max_headers;
    proof_out[2] = trusted_block;
    proof_out[3] = target_block;
    memcpy(proof_out + 4, out96, 96);
    proof_out[16] = S;
    proof_out[17] = just ? jt[0].len : 0;
    proof_out[18] = tree.len;
    proof_out[19] = just ? jt[1].len : 0;
    proof_out[20] = just ? jt[2].len : 0;
    uint64_t round = 0;
    if (just) memcpy(&round, just->precommit + 37, 8);  // 0x01 || hash 32 || block 4 || round 8 || set id 8 (decoder.rs:159-200)
    proof_out[21] = round;
    for (int s = 0; s < (int)S; ++s) proof_out[VX_HR_BLOB_FIXED_WORDS + s] = seg[s].len;
    return VX_OK;
}

extern "C" {

int32_t vx_header_range_proof_bound(const vx_stark_config* cfg, size_t n_chunks, size_t n_authorities, size_t* n_words) {
    if (!cfg || !n_words || n_chunks == 0) return VX_ERR_ARG;
    const size_t n_sig = sig_quorum(n_authorities);
    size_t w1 = 0, w2 = 0, w3 = 0, w4 = 0, w5 = 0;
    int32_t rc = vx_stark_proof_bound(VX_AIR_BLAKE_CHAIN, cfg, blake_log_n(n_chunks), &w1);
    if (rc == VX_OK && n_authorities) rc = vx_stark_proof_bound(VX_AIR_SHA_CHAIN, cfg, sha_log_n(n_authorities), &w2);
    if (rc == VX_OK) rc = vx_stark_proof_bound(tree_air_id(512), cfg, tree_log_n(512), &w3);  // the largest Merkle AIR (the request's max_headers is not known here)
    if (rc == VX_OK && n_authorities) rc = vx_stark_proof_bound(ed_air_id(n_sig), cfg, ed_log_n(n_sig), &w4);
    if (rc == VX_OK && n_authorities) rc = vx_stark_proof_bound(s512_air_id(n_sig), cfg, s512_log_n(n_sig), &w5);
    *n_words = w1 + w2 + w3 + w4 + w5 + VX_HR_HDR;
    return rc;
}
int32_t vx_header_range_prove(vx_ctx* ctx, const vx_buf* headers, size_t stride, const uint32_t* sizes, size_t n_fetched,
                              uint32_t max_headers, uint32_t trusted_block, const uint8_t trusted_hash[32], uint32_t target_block,
                              const vx_justification* just, const vx_stark_config* cfg, uint8_t out96[96], uint64_t* proof_out,
                              size_t proof_cap, size_t* proof_len) {
    return hr_prove(ctx, headers, stride, sizes, n_fetched, max_headers, trusted_block, trusted_hash, target_block, just, cfg, 1, 0, 1, nullptr, out96, proof_out, proof_cap, proof_len);
}
int32_t vx_header_range_prove_ex(vx_ctx* ctx, const vx_buf* headers, size_t stride, const uint32_t* sizes, size_t n_fetched, uint32_t max_headers, uint32_t trusted_block,
                                 const uint8_t trusted_hash[32], uint32_t target_block, const vx_justification* just, const vx_stark_config* cfg, uint32_t n_segments,
                                 uint32_t shard, uint32_t n_shards, const vx_hr_exchange* exchange, uint8_t out96[96], uint64_t* proof_out, size_t proof_cap, size_t* proof_len) {
    return hr_prove(ctx, headers, stride, sizes, n_fetched, max_headers, trusted_block, trusted_hash, target_block, just, cfg, n_segments, shard, n_shards, exchange, out96,
                    proof_out, proof_cap, proof_len);
}
int32_t vx_header_range_proof_bound_ex(const vx_stark_config* cfg, size_t n_chunks, size_t n_authorities, uint32_t n_segments, size_t* n_words) {
    if (!cfg || !n_words || n_chunks == 0 || n_segments < 1 || n_segments > VX_HR_MAX_SEGMENTS) return VX_ERR_ARG;
    size_t one = 0;
    // a segment is never taller than the unsegmented table: S copies of that bound (generous), plus the longer header
    const int32_t rc = vx_header_range_proof_bound(cfg, n_chunks, n_authorities, &one);
    size_t w1 = 0;
    int32_t rc2 = vx_stark_proof_bound(VX_AIR_BLAKE_CHAIN, cfg, blake_log_n(n_chunks), &w1);
    *n_words = one + (size_t)(n_segments - 1) * w1 + n_segments;
    return rc != VX_OK ? rc : rc2;
}
// host only: the blobs of the shards of one proof -> the request's blob
int32_t vx_header_range_merge(const uint64_t** blobs, const size_t* lens, size_t n_blobs, uint64_t* out, size_t out_cap, size_t* out_len, char* err, size_t errlen) {
    auto bad = [&](const char* why) {
        if (err && errlen) snprintf(err, errlen, "%s", why);
        return (int32_t)VX_ERR_STATEMENT;
    };
    if (!blobs || !lens || !out_len || n_blobs == 0) return VX_ERR_ARG;
    for (size_t k = 0; k < n_blobs; ++k)
        if (!blobs[k] || lens[k] <= VX_HR_BLOB_FIXED_WORDS || blobs[k][0] != VX_HR_MAGIC) return bad("merge: not a header_range blob");
    const uint64_t S = blobs[0][16];
    if (S < 1 || S > VX_HR_MAX_SEGMENTS) return bad("merge: bad segment count");
    const size_t HDR = VX_HR_BLOB_FIXED_WORDS + S, NT = S + 4;
    // table lengths of blob k in blob order: segments, commitment, Merkle, Ed25519, SHA-512
    auto tlen = [&](size_t k, size_t t) -> uint64_t { return t < S ? blobs[k][VX_HR_BLOB_FIXED_WORDS + t] : blobs[k][17 + (t - S)]; };
    std::vector<int> src(NT, -1);
    std::vector<std::vector<size_t>> offs(n_blobs, std::vector<size_t>(NT, 0));
    for (size_t k = 0; k < n_blobs; ++k) {
        if (lens[k] < HDR || blobs[k][16] != S || memcmp(blobs[k], blobs[0], 16 * 8) != 0 || blobs[k][21] != blobs[0][21]) return bad("merge: the blobs are not shards of one proof");
        size_t off = HDR;
        for (size_t t = 0; t < NT; ++t) {
            const uint64_t l = tlen(k, t);
            if (l > lens[k] - off) return bad("merge: blob lengths are inconsistent");
            offs[k][t] = off, off += l;
            if (l) {
                if (src[t] >= 0) return bad("merge: a table is present in two shards");
                src[t] = (int)k;
            }
        }
        if (off != lens[k]) return bad("merge: blob lengths are inconsistent");
    }
    size_t total = HDR;
    for (size_t t = 0; t < NT; ++t)
        if (src[t] >= 0) total += tlen(src[t], t);
    *out_len = total;
    if (!out || out_cap < total) return VX_ERR_BUFSZ;
    memcpy(out, blobs[0], HDR * 8);
    size_t off = HDR;
    for (size_t t = 0; t < NT; ++t) {
        const uint64_t l = src[t] >= 0 ? tlen(src[t], t) : 0;
        if (t < S) out[VX_HR_BLOB_FIXED_WORDS + t] = l;
        else out[17 + (t - S)] = l;
        if (l) memcpy(out + off, blobs[src[t]] + offs[src[t]][t], l * 8), off += l;
    }
    return VX_OK;
}
}
