// The generic bus group (include/vx.h "A generic bus group"): ANY admitted tables proven together on one logUp bus -- one TableGroup
// (vx_bus.h) of gen-less tables in the caller's order -- and the native statement check such a group has, the bus balance on the
// device (bus_balance.cuh: the records kernels, the sort, the match).  The verifier is vx_bus_group_verify in vx_verify.hip.
#include <stdio.h>
#include <string.h>

#include "air_program.h"
#include "bus_balance.cuh"
#include "vx_bus.h"

namespace {
const char* const WHAT = "bus group";

// admission and the arguments of a table, on `ctx`
int32_t group_tables(vx_ctx* ctx, const vx_bus_table* t, size_t n, BusAirShape* shape) {
    int32_t ids[VX_BUS_GROUP_MAX_TABLES];
    size_t n_pub[VX_BUS_GROUP_MAX_TABLES];
    for (size_t k = 0; k < n && k < (size_t)VX_BUS_GROUP_MAX_TABLES; ++k) ids[k] = t[k].air_id, n_pub[k] = t[k].n_public;
    char why[200] = "";
    if (const int32_t rc = vx_bus_group_admit(ids, n_pub, n, shape, why, sizeof why)) return vx_fail(ctx, rc, "%s", why);
    for (size_t k = 0; k < n; ++k) {
        VX_CHECK(t[k].log_n >= 2 && t[k].log_n <= 26, "bus group: table %zu has 2^%d rows (2^2 .. 2^26)", k, t[k].log_n);
        VX_CHECK(t[k].trace && t[k].trace->n == (size_t)shape[k].cols << t[k].log_n, "bus group: the trace of table %zu is not cols << log_n words", k);
        VX_CHECK(t[k].n_public == (size_t)shape[k].pub && (t[k].n_public == 0 || t[k].public_inputs), "bus group: table %zu (air %d) takes %d public inputs, %zu given", k, t[k].air_id,
                 shape[k].pub, t[k].n_public);
        for (size_t q = 0; q < t[k].n_public; ++q) VX_CHECK(t[k].public_inputs[q] < glh::P, "bus group: table %zu has a non-canonical public input at %zu", k, q);
    }
    return VX_OK;
}
int32_t group_outside(vx_ctx* ctx, const uint64_t* outside, size_t n_outside) {
    char why[200] = "";
    if (const int32_t rc = vx_bus_outside_ok(outside, n_outside, VX_ERR_ARG, why, sizeof why)) return vx_fail(ctx, rc, "%s", why);
    return VX_OK;
}
// rows that share one set of messages in table k (1 or 32); 0: the table has no message list
int message_rows(const vx_bus_table& t, const BusAirShape& sh) {
    if (sh.prog) return sh.prog->bus_help > 0 ? 1 << sh.prog->bus_block_log : 0;
    return bus_records_rows(t.air_id, VxAirs{});
}
size_t words_of(size_t bytes) { return (bytes + 7) / 8; }

// The balance check of admitted tables that all have a message list.  Everything comes from the context's pool.  The host waits twice:
// for the ONE word that says how many records there are -- the sort takes its length from the host -- and at the end.
int32_t bus_balance_dev(vx_ctx* ctx, const vx_bus_table* t, const BusAirShape* shape, size_t n, const uint64_t* outside, size_t n_outside, vx_bus_unmatched* out) {
    *out = vx_bus_unmatched{0, 0, 0, 0, 0};
    size_t lane0[VX_BUS_GROUP_MAX_TABLES + 1] = {0};  // where the lanes of table k start in cnt / offs
    for (size_t k = 0; k < n; ++k) {
        const int rows = message_rows(t[k], shape[k]);
        VX_CHECK(rows > 0, "bus group: table %zu (air %d) has no message list (a vx_air_register_bus program or a compiled AIR 4, 7 .. 9, 11, 13 .. 23 has one)", k, t[k].air_id);
        VX_CHECK(((size_t)1 << t[k].log_n) >= (size_t)rows, "bus group: table %zu has 2^%d rows, less than one block of its bus", k, t[k].log_n);
        lane0[k + 1] = lane0[k] + (((size_t)1 << t[k].log_n) / rows);
    }
    const size_t lanes = lane0[n];
    // the outside party's records, on the host: the denominator under the check challenges
    std::vector<uint64_t> orec[4];
    {
        const Fx beta{BUS_CHECK_CHAL[0], BUS_CHECK_CHAL[1]}, gamma{BUS_CHECK_CHAL[2], BUS_CHECK_CHAL[3]}, g2 = gamma * gamma, g3 = g2 * gamma, g4 = g2 * g2;
        for (size_t i = 0; i < n_outside; ++i) {
            const uint64_t* w = outside + i * VX_BUS_MSG_WORDS;
            if (!w[5]) continue;
            const Fx d = beta + Fx{w[0], 0} + fx_scale(gamma, w[1]) + fx_scale(g2, w[2]) + fx_scale(g3, w[3]) + fx_scale(g4, w[4]);
            orec[0].push_back(d.a), orec[1].push_back(d.b), orec[2].push_back(w[5]), orec[3].push_back(bus_origin(n, i, 0));
        }
    }
    const size_t n_out = orec[0].size();
    // ---- the count pass and the scan
    std::vector<uint64_t> blob;  // the message programs of the run-time tables, one upload
    size_t blob_at[VX_BUS_GROUP_MAX_TABLES] = {0};
    for (size_t k = 0; k < n; ++k)
        if (shape[k].prog) blob_at[k] = blob.size(), busp_blob(*shape[k].prog, t[k].public_inputs, blob);
    size_t scan_bytes = 0;
    VX_HIP(rocprim::exclusive_scan(nullptr, scan_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t)0, lanes + 1, rocprim::plus<uint64_t>(), ctx->stream));
    Scratch a;
    uint64_t *cnt = nullptr, *offs = nullptr, *scan_tmp = nullptr, *blob_d = nullptr;
    a.add(scan_tmp, words_of(scan_bytes) + 1);  // (first: rocPRIM carves its storage assuming the alignment of an allocation)
    a.add(cnt, lanes + 1), a.add(offs, lanes + 1), a.add(blob_d, blob.size() + 1);
    a.alloc(ctx);
    if (!blob.empty()) a.up(blob_d, blob.data(), blob.size() * 8);
    a.fill(cnt + lanes, 0, 8);  // (the scan runs one past the lanes: offs[lanes] is the number of records)
    if (!a.ok()) return a.status(WHAT);
    const BusRecords none{nullptr, nullptr, nullptr, nullptr};
    auto pass = [&](auto emit, const BusRecords& rec, uint64_t n_rec) {
        constexpr bool EMIT = decltype(emit)::value;
        for (size_t k = 0; k < n; ++k) {
            const size_t rows = (size_t)1 << t[k].log_n;
            if (shape[k].prog) {
                const AirProgram& pg = *shape[k].prog;
                const size_t l = rows >> pg.bus_block_log;
                hipLaunchKernelGGL((k_bus_records_prog<EMIT>), dim3((unsigned)((l + BUSP_BLOCK - 1) / BUSP_BLOCK)), dim3(BUSP_BLOCK), (size_t)pg.bus_regs * BUSP_BLOCK * sizeof(uint64_t),
                                   ctx->stream, t[k].trace->d, rows, busp_args(pg, blob_d + blob_at[k]), cnt + lane0[k], offs + lane0[k], rec, n_rec, (uint64_t)k);
            } else {
                (void)bus_records_launch<EMIT>(t[k].air_id, VxAirs{}, ctx->stream, t[k].trace->d, rows, t[k].public_inputs, cnt + lane0[k], offs + lane0[k], rec, n_rec, (uint64_t)k);
            }
            a.launched();
        }
    };
    pass(std::false_type{}, none, 0);
    if (a.ok()) a.keep(rocprim::exclusive_scan(scan_tmp, scan_bytes, cnt, offs, (uint64_t)0, lanes + 1, rocprim::plus<uint64_t>(), ctx->stream));
    uint64_t n_tab = 0;
    a.down(&n_tab, offs + lanes, 8);
    a.sync();  // (blob, a host vector, has outlived its copy)
    if (!a.ok()) return a.status(WHAT);
    const size_t N = (size_t)n_tab + n_out;
    if (N == 0) return VX_OK;  // nobody says anything: the bus closes
    // ---- the records, their order, the match
    size_t sort_bytes = 0, sb = 0;
    VX_HIP(rocprim::radix_sort_pairs(nullptr, sort_bytes, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr, (uint64_t*)nullptr, N, 0, 64, ctx->stream));
    Scratch b;
    BusRecords rec{};
    uint64_t *iota = nullptr, *k1 = nullptr, *p1 = nullptr, *hi_g = nullptr, *hi_s = nullptr, *p2 = nullptr, *lo_s = nullptr, *m_s = nullptr, *org_s = nullptr, *net_of = nullptr,
             *low_of = nullptr, *sort_tmp = nullptr, *res = nullptr;
    b.add(sort_tmp, words_of(sort_bytes) + 1);  // (first, as above)
    for (uint64_t** p : {&rec.hi, &rec.lo, &rec.m, &rec.origin, &iota, &k1, &p1, &hi_g, &hi_s, &p2, &lo_s, &m_s, &org_s, &net_of, &low_of}) b.add(*p, N);
    b.add(res, 4);
    b.alloc(ctx);
    if (!b.ok()) return b.status(WHAT);
    pass(std::true_type{}, rec, n_tab);
    b.keep(a.err);
    for (int f = 0; f < 4 && n_out; ++f) b.up((f == 0 ? rec.hi : f == 1 ? rec.lo : f == 2 ? rec.m : rec.origin) + n_tab, orec[f].data(), n_out * 8);
    b.fill(net_of, 0, N * 8), b.fill(res, 0, 32), b.fill(res + 1, 0xFF, 8);
    const dim3 grid((unsigned)((N + BUS_MATCH_BLOCK - 1) / BUS_MATCH_BLOCK)), blk(BUS_MATCH_BLOCK);
    const BusGather g_hi{{rec.hi, nullptr, nullptr}, {hi_g, nullptr, nullptr}, 1}, g_rest{{rec.lo, rec.m, rec.origin}, {lo_s, m_s, org_s}, 3};
    if (b.ok()) {
        hipLaunchKernelGGL(k_bus_iota, grid, blk, 0, ctx->stream, iota, N);
        b.launched();
        sb = sort_bytes;
        b.keep(rocprim::radix_sort_pairs(sort_tmp, sb, rec.lo, k1, iota, p1, N, 0, 64, ctx->stream));  // stable: the low word first
        hipLaunchKernelGGL(k_bus_gather, grid, blk, 0, ctx->stream, g_hi, p1, N);
        b.launched();
        sb = sort_bytes;
        b.keep(rocprim::radix_sort_pairs(sort_tmp, sb, hi_g, hi_s, p1, p2, N, 0, 64, ctx->stream));  // ... then the high one
        hipLaunchKernelGGL(k_bus_gather, grid, blk, 0, ctx->stream, g_rest, p2, N);
        hipLaunchKernelGGL(k_bus_match, grid, blk, 0, ctx->stream, hi_s, lo_s, m_s, org_s, N, (unsigned long long*)res, net_of, low_of);
        hipLaunchKernelGGL(k_bus_net, grid, blk, 0, ctx->stream, net_of, low_of, N, (unsigned long long*)res);
        b.launched();
    }
    uint64_t got[3] = {0, 0, 0};
    b.down(got, res, 24);
    b.sync();  // (orec, host vectors, have outlived their copies; the pool blocks the kernels)
    if (!b.ok()) return b.status(WHAT);
    if (got[0]) *out = vx_bus_unmatched{got[0], (int32_t)(got[1] >> 56), (uint32_t)(got[1] & 0xFF), (got[1] >> 8) & 0xFFFFFFFFFFFFull, got[2]};
    return VX_OK;
}
}  // namespace

extern "C" {
int32_t vx_bus_group_proof_bound(const vx_stark_config* cfg, const vx_bus_table* tables, size_t n, size_t* n_words) {
    if (!cfg || !tables || !n_words) return VX_ERR_ARG;
    int32_t ids[VX_BUS_GROUP_MAX_TABLES];
    TableShape sh[VX_BUS_GROUP_MAX_TABLES];
    for (size_t k = 0; k < n && k < (size_t)VX_BUS_GROUP_MAX_TABLES; ++k) ids[k] = tables[k].air_id, sh[k] = {tables[k].air_id, tables[k].log_n};
    VX_TRY(vx_bus_group_admit(ids, nullptr, n, nullptr, nullptr, 0));
    return vx_tables_proof_bound(cfg, VX_BGRP_HDR + n, sh, n, n_words);
}

int32_t vx_bus_group_check(vx_ctx* ctx, const vx_bus_table* tables, size_t n, const uint64_t* outside, size_t n_outside, vx_bus_unmatched* out) {
    if (!ctx || !tables || !out) return VX_ERR_ARG;
    BusAirShape shape[VX_BUS_GROUP_MAX_TABLES];
    VX_TRY(group_tables(ctx, tables, n, shape));
    VX_TRY(group_outside(ctx, outside, n_outside));
    return bus_balance_dev(ctx, tables, shape, n, outside, n_outside, out);
}

int32_t vx_bus_group_prove(vx_ctx* ctx, const vx_stark_config* cfg, const vx_bus_table* tables, size_t n, const uint64_t* outside, size_t n_outside, uint64_t* blob_out, size_t blob_cap,
                           size_t* blob_len) {
    if (!ctx || !cfg || !tables || !blob_len) return VX_ERR_ARG;
    *blob_len = 0;
    BusAirShape shape[VX_BUS_GROUP_MAX_TABLES];
    VX_TRY(group_tables(ctx, tables, n, shape));
    VX_TRY(group_outside(ctx, outside, n_outside));
    bool lists = true;
    for (size_t k = 0; k < n; ++k) lists = lists && message_rows(tables[k], shape[k]) > 0;
    if (lists) {  // the native statement check of a generic group: what is wrong is named before anything is proven
        vx_bus_unmatched u;
        VX_TRY(bus_balance_dev(ctx, tables, shape, n, outside, n_outside, &u));
        if (u.n_unmatched && (size_t)u.table >= n)
            return vx_fail(ctx, VX_ERR_STATEMENT, "bus group: the bus does not close: outside message %llu has no partner (net multiplicity %llu; %llu unmatched tuples)",
                           (unsigned long long)u.row, (unsigned long long)u.net, (unsigned long long)u.n_unmatched);
        if (u.n_unmatched)
            return vx_fail(ctx, VX_ERR_STATEMENT, "bus group: the bus does not close: message %u of table %d (air %d) at row %llu has no partner (net multiplicity %llu; %llu unmatched tuples)",
                           u.message, u.table, tables[u.table].air_id, (unsigned long long)u.row, (unsigned long long)u.net, (unsigned long long)u.n_unmatched);
    }
    VX_HIP(vx_wait(ctx));  // the traces were written on ctx's stream; the side contexts may have streams of their own
    char names[VX_BUS_GROUP_MAX_TABLES][24];
    TableGroup g(ctx, cfg, WHAT);
    for (size_t k = 0; k < n; ++k) {
        snprintf(names[k], sizeof names[k], "table %zu", k);
        TableSpec s{names[k], tables[k].air_id, tables[k].log_n, (size_t)shape[k].cols, tables[k].n_public, 0, nullptr};
        s.trace = const_cast<vx_buf*>(tables[k].trace), s.pub = tables[k].public_inputs;  // (consume_trace 0: the trace is read only)
        g.add(std::move(s));
    }
    VX_TRY(g.prove(0));
    const TableJob* jobs[VX_BUS_GROUP_MAX_TABLES];
    for (size_t k = 0; k < n; ++k) jobs[k] = &g.job[k];
    if (!lists) {  // no check before: the published totals and the outside messages must cancel
        const uint64_t* proofs[VX_BUS_GROUP_MAX_TABLES];
        size_t lens[VX_BUS_GROUP_MAX_TABLES];
        for (size_t k = 0; k < n; ++k) proofs[k] = g.job[k].proof.data(), lens[k] = g.job[k].len;
        char why[200] = "";
        if (const int32_t rc = vx_bus_group_closes(cfg, proofs, lens, n, outside, n_outside, why, sizeof why)) return vx_fail(ctx, rc, "%s", why);
    }
    const uint64_t request[1] = {(uint64_t)n};
    return pack_blob(ctx, WHAT, VX_BGRP_MAGIC, request, 1, jobs, n, blob_out, blob_cap, blob_len);
}
}  // extern "C"
