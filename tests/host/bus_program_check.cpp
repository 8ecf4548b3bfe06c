// The checks and the lowering of declared bus messages (0-kno-vectorx_amd/csrc/bus_program.h) on a CPU, with no library and no
// GPU: the message programs of tests/golden/bus_programs.txt (written by tests/golden/make_bus_programs.py) are lowered, the lowered
// code is run by air_program_eval over the base field on random rows, and every constraint it asserts is compared with a DIRECT
// evaluation in the extension field -- h D_a D_b - m_a D_b - m_b D_a per helper, then z' - z - sum h [* per[step]] + total -- from
// an independent reading of the message program.  Then every refusal, every truncation of a fixture program and a few thousand
// seeded random programs go through validation; what it admits is lowered and run.  Meant to run under the address and
// undefined-behaviour sanitizers: every array below has exactly the length the declaration states.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>

#include "../../0-kno-vectorx_amd/csrc/bus_program.h"
#include "../../0-kno-vectorx_amd/csrc/glh.h"

namespace {
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) {                                          \
            printf("FAILED %s:%d: %s: ", __FILE__, __LINE__, #cond); \
            printf(__VA_ARGS__);                                \
            printf("\n");                                       \
            exit(1);                                            \
        }                                                       \
    } while (0)

struct F {  // the base field, for air_program_eval
    uint64_t v;
    F operator+(F o) const { return {glh::add(v, o.v)}; }
    F operator-(F o) const { return {glh::sub(v, o.v)}; }
    F operator*(F o) const { return {glh::mul(v, o.v)}; }
    static F from(uint64_t x) { return {x % glh::P}; }
};
struct Collect {  // the constraint consumer: keeps what is asserted, and how
    std::vector<F> out;
    int not_plain = 0;
    void constraint(F c) { out.push_back(c); }
    void transition(F c) { out.push_back(c), ++not_plain; }
    void first_row(F c) { out.push_back(c), ++not_plain; }
    void last_row(F c) { out.push_back(c), ++not_plain; }
};
uint64_t rng_state = 0x243F6A8885A308D3ULL;
uint64_t rnd() {  // SplitMix64
    uint64_t z = (rng_state += 0x9E3779B97F4A7C15ULL);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
uint64_t rnd_field() {
    const uint64_t r = rnd();
    switch (r & 15) {  // the edges now and then
        case 0: return 0;
        case 1: return 1;
        case 2: return glh::P - 1;
        default: return (r >> 4) % glh::P;
    }
}
std::vector<F> rnd_row(size_t n) {
    std::vector<F> r(n);
    for (F& x : r) x = {rnd_field()};
    return r;
}

struct Prog {
    std::string name;
    uint32_t cols = 0, n_public = 0, block_log = 0, n_regs = 0;
    int32_t step = -1;
    std::vector<uint8_t> plog;
    std::vector<uint64_t> pvals, consts, code;
    uint32_t messages() const {
        uint32_t m = 0;
        for (uint64_t w : code) m += (w & 0xFF) == VX_BUSP_MSG;
        return m;
    }
};
const uint64_t OWN[2] = {busp::insn(VX_AIRP_LOC, 0, 0), busp::insn(VX_AIRP_ASSERT, 0, 0)};  // the program's own constraint: column 0
struct Decl {  // a Prog as the two structs of the C ABI
    vx_air_program in{};
    vx_air_bus bus{};
    explicit Decl(const Prog& p) {
        const uint32_t h = (p.messages() + 1) / 2;
        in.cols = p.cols, in.n_public = p.n_public, in.n_periodic = (uint32_t)p.plog.size(), in.n_regs = 1;
        in.periodic_log = p.plog.data(), in.periodic_values = p.pvals.data();
        in.code = OWN, in.n_code = 2, in.aux_cols = 2 * h + 2, in.n_challenges = 4, in.n_aux_public = 1;
        bus.code = p.code.data(), bus.n_code = (uint32_t)p.code.size(), bus.consts = p.consts.data(), bus.n_consts = (uint32_t)p.consts.size();
        bus.n_regs = p.n_regs, bus.block_log = p.block_log, bus.step_periodic = p.step;
    }
};

std::vector<Prog> read_fixture(const char* path) {
    std::ifstream f(path);
    CHECK(f.good(), "cannot open %s", path);
    size_t n = 0;
    f >> n;
    std::vector<Prog> out(n);
    for (Prog& p : out) {
        size_t k = 0;
        f >> p.name >> p.cols >> p.n_public >> p.block_log >> p.step >> p.n_regs;
        f >> k;
        p.plog.resize(k);
        for (uint8_t& x : p.plog) {
            unsigned v;
            f >> v;
            x = (uint8_t)v;
        }
        f >> k;
        p.pvals.resize(k);
        for (uint64_t& x : p.pvals) f >> x;
        f >> k;
        p.consts.resize(k);
        for (uint64_t& x : p.consts) f >> x;
        f >> k;
        p.code.resize(k);
        for (uint64_t& x : p.code) f >> x;
        CHECK(!f.fail(), "fixture truncated in program %s", p.name.c_str());
    }
    return out;
}

// lowers a VALID declaration and runs the lowered code on `rounds` random rows against the direct evaluation -> constraints per row
size_t lower_and_compare(const Prog& p, int rounds) {
    const Decl d(p);
    char err[256] = "";
    uint32_t n_msgs = 0;
    CHECK(busp::validate(d.in, d.bus, &n_msgs, err, sizeof err), "%s: refused: %s", p.name.c_str(), err);
    CHECK(n_msgs == p.messages() && err[0] == 0, "%s", p.name.c_str());
    busp::Lowered lo;
    busp::lower(d.in, d.bus, n_msgs, &lo);
    const uint32_t H = (n_msgs + 1) / 2;
    CHECK(lo.n_help == H && lo.n_regs <= VX_AIRP_MAX_REGS && lo.n_regs == p.n_regs + VX_BUSP_LOWER_REGS, "%s: %u registers", p.name.c_str(), lo.n_regs);
    AirProgram ap;
    ap.n_regs = lo.n_regs, ap.code = lo.code, ap.consts = lo.consts;
    for (uint64_t w : lo.code) {  // ordinary instructions only, every register inside the file
        const AirpInsn i = airp_decode(w);
        CHECK(i.op >= VX_AIRP_LOC && i.op <= VX_AIRP_APUB && i.d < (int)lo.n_regs, "%s: lowered opcode %d", p.name.c_str(), i.op);
        if (i.op >= VX_AIRP_ADD && i.op <= VX_AIRP_MUL) CHECK(i.a < (int)lo.n_regs && i.b < (int)lo.n_regs, "%s", p.name.c_str());
        if (i.op == VX_AIRP_CONST) CHECK(i.a < (int)lo.consts.size() && lo.consts[i.a] < glh::P, "%s", p.name.c_str());
    }
    const size_t width = p.cols + 2 * H + 2;
    for (int round = 0; round < rounds; ++round) {
        const std::vector<F> loc = rnd_row(width), nxt = rnd_row(width), per = rnd_row(p.plog.size()), pub = rnd_row(p.n_public), chal = rnd_row(4), apub = rnd_row(2);
        Collect got;
        air_program_eval<F>(ap, loc, nxt, per.data(), pub.data(), chal.data(), apub.data(), got);
        CHECK(got.not_plain == 0 && got.out.size() == 1 + 2 * H + 2, "%s: %zu constraints", p.name.c_str(), got.out.size());
        CHECK(got.out[0].v == loc[0].v, "%s: the program's own constraint", p.name.c_str());
        // the direct evaluation: an independent reading of the message program
        const Fx beta{chal[0].v, chal[1].v}, gamma{chal[2].v, chal[3].v}, g2 = gamma * gamma, g3 = g2 * gamma, g4 = g2 * g2;
        std::vector<uint64_t> r(p.n_regs, 0);
        std::vector<Fx> den;
        std::vector<uint64_t> mult;
        Fx D = beta;
        for (uint64_t w : p.code) {
            const AirpInsn i = airp_decode(w);
            switch (i.op) {
                case VX_AIRP_LOC: r[i.d] = loc[i.a].v; break;
                case VX_AIRP_PER: r[i.d] = per[i.a].v; break;
                case VX_AIRP_PUB: r[i.d] = pub[i.a].v; break;
                case VX_AIRP_CONST: r[i.d] = p.consts[i.a]; break;
                case VX_AIRP_ADD: r[i.d] = glh::add(r[i.a], r[i.b]); break;
                case VX_AIRP_SUB: r[i.d] = glh::sub(r[i.a], r[i.b]); break;
                case VX_AIRP_MUL: r[i.d] = glh::mul(r[i.a], r[i.b]); break;
                case VX_BUSP_SLOT: D = D + fx_scale(i.d == 0 ? Fx{1, 0} : i.d == 1 ? gamma : i.d == 2 ? g2 : g3, r[i.a]); break;
                case VX_BUSP_MSG:
                    den.push_back(D + fx_scale(g4, (uint64_t)i.b)), mult.push_back(r[i.a]);
                    D = beta;
                    break;
                default: CHECK(false, "%s: opcode %d in a validated message program", p.name.c_str(), i.op);
            }
        }
        Fx hsum{0, 0};
        for (uint32_t e = 0; e < H; ++e) {
            const Fx h{loc[p.cols + 2 * e].v, loc[p.cols + 2 * e + 1].v};
            hsum = hsum + h;
            Fx want;
            if (2 * e + 1 < n_msgs) want = h * den[2 * e] * den[2 * e + 1] - fx_scale(den[2 * e + 1], mult[2 * e]) - fx_scale(den[2 * e], mult[2 * e + 1]);
            else want = h * den[2 * e] - Fx{mult[2 * e], 0};
            CHECK(got.out[1 + 2 * e].v == want.a && got.out[2 + 2 * e].v == want.b, "%s: helper %u (round %d)", p.name.c_str(), e, round);
        }
        const size_t Z = p.cols + 2 * H;
        const Fx z{loc[Z].v, loc[Z + 1].v}, zn{nxt[Z].v, nxt[Z + 1].v}, total{apub[0].v, apub[1].v};
        const Fx want = zn - z - (p.block_log ? fx_scale(hsum, per[p.step].v) : hsum) + total;
        CHECK(got.out[1 + 2 * H].v == want.a && got.out[2 + 2 * H].v == want.b, "%s: the running sum (round %d)", p.name.c_str(), round);
    }
    return 1 + 2 * H + 2;
}

// ---- refusals: one valid declaration, one change each
uint64_t I(int op, int d = 0, int a = 0, int b = 0) { return busp::insn(op, d, a, b); }
Prog base() {
    Prog p;
    p.name = "base", p.cols = 2, p.n_public = 1, p.n_regs = 2;
    p.code = {I(VX_AIRP_LOC, 0, 0), I(VX_BUSP_SLOT, 0, 0), I(VX_AIRP_LOC, 1, 1), I(VX_BUSP_MSG, 0, 1, 3)};
    return p;
}
void refused(const Prog& p, const char* why, void (*change)(Decl&) = nullptr) {
    Decl d(p);
    if (change) change(d);
    char err[256] = "";
    uint32_t n_msgs = 77;
    CHECK(!busp::validate(d.in, d.bus, &n_msgs, err, sizeof err), "admitted: %s", why);
    CHECK(strstr(err, why) && n_msgs == 77, "the refusal \"%s\" does not name its cause \"%s\"", err, why);
    CHECK(!busp::validate(d.in, d.bus, &n_msgs, nullptr, 0), "%s: no buffer", why);  // a caller that wants no text
    char tiny[8];
    CHECK(!busp::validate(d.in, d.bus, &n_msgs, tiny, sizeof tiny) && strlen(tiny) < sizeof tiny, "%s: a short buffer", why);
}
int32_t a_callback(void*, vx_ctx*, const vx_buf*, int, const uint64_t*, const uint64_t*, vx_buf*, uint64_t*) { return 0; }
void refusals() {
    lower_and_compare(base(), 4);
    auto with_code = [](std::vector<uint64_t> code, uint32_t n_regs = 2) {
        Prog p = base();
        p.code = code, p.n_regs = n_regs;
        return p;
    };
    const std::vector<uint64_t> one = base().code;
    auto before = [&](uint64_t w) {
        std::vector<uint64_t> c{w};
        c.insert(c.end(), one.begin(), one.end());
        return c;
    };
    auto after = [&](uint64_t w) {
        std::vector<uint64_t> c(one);
        c.push_back(w);
        return c;
    };
    refused(base(), "gen_aux callback given together with a bus", [](Decl& d) { d.in.gen_aux = a_callback; });
    refused(base(), "need aux_cols 4", [](Decl& d) { d.in.aux_cols = 6; });
    refused(base(), "n_challenges 4", [](Decl& d) { d.in.n_challenges = 2; });
    refused(base(), "n_aux_public 1", [](Decl& d) { d.in.n_aux_public = 0; });
    refused(with_code(before(I(VX_AIRP_NXT, 0, 0))), "NXT is not allowed");
    refused(with_code(before(I(VX_AIRP_CHAL, 0, 0))), "CHAL is not allowed");
    refused(with_code(before(I(VX_AIRP_APUB, 0, 0))), "APUB is not allowed");
    for (int op = VX_AIRP_ASSERT; op <= VX_AIRP_ASSERT_LAST; ++op) refused(with_code(after(I(op, 0, 0))), "an assert is not allowed");
    refused(with_code(before(I(15, 0, 0))), "unknown opcode 15");
    refused(with_code(before(I(0, 0, 0))), "unknown opcode 0");
    refused(with_code(after(I(66, 0, 0))), "unknown opcode 66");
    refused(with_code(before(I(VX_AIRP_LOC, 0, 2))), "LOC of an auxiliary column");
    refused(with_code(before(I(VX_AIRP_LOC, 0, 6))), "bad column load");
    refused(with_code(before(I(VX_AIRP_LOC, 2, 0))), "bad column load");
    refused(with_code(before(I(VX_AIRP_PER, 0, 0))), "bad periodic load");
    refused(with_code(before(I(VX_AIRP_PUB, 0, 1))), "bad public-input load");
    refused(with_code(before(I(VX_AIRP_CONST, 0, 0))), "bad constant load");
    refused(with_code({I(VX_AIRP_LOC, 0, 0), I(VX_BUSP_SLOT, 4, 0), I(VX_BUSP_MSG, 0, 0, 3)}), "slot index 4 above 3");
    refused(with_code({I(VX_AIRP_LOC, 0, 0), I(VX_BUSP_SLOT, 1, 0), I(VX_BUSP_SLOT, 1, 0), I(VX_BUSP_MSG, 0, 0, 3)}), "twice");
    refused(with_code(after(I(VX_BUSP_SLOT, 1, 0))), "SLOT not followed by a MSG");
    refused(with_code({I(VX_AIRP_LOC, 0, 0)}), "no message");
    {
        Prog p = base();
        for (int k = 0; k < 2 * VX_BUSP_MAX_HELPERS; ++k) p.code.insert(p.code.end(), one.begin(), one.end());
        refused(p, "more than 19 helpers");
        p.code.resize(p.code.size() - one.size());
        CHECK(lower_and_compare(p, 2) == 1 + 2 * VX_BUSP_MAX_HELPERS + 2, "the largest table");
    }
    {
        Prog p = with_code(before(I(VX_AIRP_CONST, 0, 0)));
        p.consts = {glh::P};
        refused(p, "non-canonical constant");
        p.consts = {glh::P - 1};
        lower_and_compare(p, 2);
    }
    refused(with_code(before(I(VX_AIRP_ADD, 0, 0, 1))), "never written");
    refused(with_code(before(I(VX_AIRP_MUL, 0, 2, 0))), "never written");
    refused(with_code({I(VX_BUSP_MSG, 0, 0, 3)}), "never written");
    refused(with_code(before(I(VX_BUSP_SLOT, 0, 5)), 8), "never written");
    refused(with_code(one, 0), "0 registers");
    refused(with_code(one, VX_BUSP_MAX_REGS + 1), "13 registers");
    refused(with_code(before(I(VX_AIRP_LOC, 0, 0) | 1ULL << 48)), "reserved bits");
    refused(with_code({I(VX_AIRP_LOC, 0, 0), I(VX_BUSP_MSG, 1, 0, 3)}), "MSG reads");
    refused(base(), "instructions", [](Decl& d) { d.bus.n_code = 0; });
    refused(base(), "instructions", [](Decl& d) { d.bus.code = nullptr; });
    // the step column
    Prog blocks = base();
    blocks.block_log = 5, blocks.step = 1, blocks.plog = {5, 5}, blocks.pvals.assign(64, 0), blocks.pvals[1] = 1, blocks.pvals[32] = 1;
    lower_and_compare(blocks, 4);
    refused(blocks, "wrong step column", [](Decl& d) { d.bus.step_periodic = 0; });   // 1 at position 1
    refused(blocks, "wrong step column", [](Decl& d) { d.bus.step_periodic = 2; });   // no such column
    refused(blocks, "wrong step column", [](Decl& d) { d.bus.step_periodic = -1; });
    refused(blocks, "wrong step column", [](Decl& d) { d.bus.block_log = 0; });       // a step column without blocks
    refused(blocks, "block_log 3 is not supported", [](Decl& d) { d.bus.block_log = 3; });
    refused(blocks, "block_log 6 is not supported", [](Decl& d) { d.bus.block_log = 6; });
    {
        Prog p = blocks;
        p.pvals[63] = 1;  // a second one
        refused(p, "wrong step column");
        p = blocks;
        p.pvals[32] = 2;
        refused(p, "wrong step column");
        p = blocks;
        p.plog = {5, 2}, p.pvals.resize(36);
        refused(p, "wrong step column");
    }
}

// ---- truncations and random programs: validation decides, and what it admits lowers and runs
size_t admitted = 0, turned_away = 0;
void try_program(const Prog& p) {
    const Decl d(p);
    char err[256] = "";
    uint32_t n_msgs = 0;
    if (busp::validate(d.in, d.bus, &n_msgs, err, sizeof err)) ++admitted, lower_and_compare(p, 1);
    else {
        CHECK(err[0] != 0, "a refusal without a reason");
        ++turned_away;
    }
}
void fuzz(const std::vector<Prog>& fixtures) {
    for (const Prog& f : fixtures)
        for (size_t len = 1; len < f.code.size(); ++len) {
            Prog p = f;
            p.code.resize(len);
            try_program(p);
        }
    const size_t after_truncations = admitted;
    CHECK(admitted > 0 && turned_away > 0, "truncations: %zu admitted, %zu refused", admitted, turned_away);
    static const int OPS[] = {VX_AIRP_LOC, VX_AIRP_LOC, VX_AIRP_PER, VX_AIRP_PUB, VX_AIRP_CONST, VX_AIRP_ADD, VX_AIRP_SUB, VX_AIRP_MUL, VX_BUSP_SLOT, VX_BUSP_SLOT, VX_BUSP_MSG, VX_BUSP_MSG,
                              VX_AIRP_NXT, VX_AIRP_ASSERT, VX_AIRP_CHAL, VX_AIRP_APUB, 0, 15, 63, 66, 255};
    for (int round = 0; round < 4000; ++round) {
        Prog p;
        p.name = "random", p.cols = 1 + rnd() % 4, p.n_public = rnd() % 3, p.n_regs = 1 + rnd() % (round % 50 ? 6 : 14);
        p.consts = {rnd_field(), glh::P - 1};
        if (round % 3 == 0) p.block_log = 5, p.step = 0, p.plog = {5, 1}, p.pvals.assign(34, 0), p.pvals[0] = 1, p.pvals[33] = 7;
        const size_t len = 1 + rnd() % 14;
        const bool wild = round % 4 == 0;  // mostly programs a builder could have written; now and then any word
        for (uint32_t k = 0; !wild && round % 8 && k < p.n_regs; ++k) p.code.push_back(I(VX_AIRP_LOC, k, rnd() % p.cols));  // (mostly) no register unwritten
        for (size_t k = 0; k < len; ++k) {
            const uint64_t r = rnd();
            const int op = wild ? OPS[r % (sizeof OPS / sizeof OPS[0])] : OPS[r % 12];
            if (wild && r >> 60 == 0) p.code.push_back(rnd());
            else if (wild) p.code.push_back(I(op, (r >> 8) % 9, (r >> 16) % 9, (r >> 24) % 9));
            else if (op == VX_BUSP_MSG) p.code.push_back(I(op, 0, (r >> 16) % p.n_regs, (r >> 24) % 400));
            else if (op == VX_BUSP_SLOT) p.code.push_back(I(op, (r >> 8) % 4, (r >> 16) % p.n_regs));
            else if (op >= VX_AIRP_ADD) p.code.push_back(I(op, (r >> 8) % p.n_regs, (r >> 16) % p.n_regs, (r >> 24) % p.n_regs));
            else p.code.push_back(I(op, (r >> 8) % p.n_regs, op == VX_AIRP_LOC ? (r >> 16) % p.cols : op == VX_AIRP_PUB ? (r >> 16) % (p.n_public + 1) : (r >> 16) % 2));
        }
        if (!wild) p.code.push_back(I(VX_BUSP_MSG, 0, rnd() % p.n_regs, rnd() % 20));
        try_program(p);
    }
    CHECK(admitted > after_truncations + 50, "random programs: only %zu admitted", admitted - after_truncations);
}
}  // namespace

int main(int argc, char** argv) {
    CHECK(argc == 2, "usage: bus_program_check tests/golden/bus_programs.txt");
    const std::vector<Prog> fixtures = read_fixture(argv[1]);
    CHECK(fixtures.size() == 5, "%zu programs", fixtures.size());
    size_t constraints = 0;
    for (const Prog& p : fixtures) constraints += lower_and_compare(p, 50);
    refusals();
    fuzz(fixtures);
    printf("ok %zu constraints, %zu admitted, %zu refused\n", constraints, admitted, turned_away);
    return 0;
}
