"""Table streams (VX_TABLE_STREAMS, csrc/vx_core.hip): a proof's tables on streams of their own ("own") or all on the one stream of
the host's context ("shared").  The mode is read when a host context is created, so one process holds both kinds: the same
requests proven on an `own` and on a `shared` context give the same bytes, the same refusals, and contexts of either kind come
and go without an error.  Shapes: the smallest every table still runs at -- Ptiny headers (a 2^16-row hash-chain table), a
16-leaf Merkle table, 4 authorities, 8 queries."""
import os
import re
import threading

import pytest

pytestmark = pytest.mark.gpu

MODES = ("own", "shared")
N_AUTH, MAX_AUTH, QUERIES = 4, 8, 8


def make_context(vx, mode):
    """A host context whose side contexts will be `mode`: the variable is read by vx_ctx_create and by nothing later."""
    old = os.environ.get("VX_TABLE_STREAMS")
    os.environ["VX_TABLE_STREAMS"] = mode
    try:
        return vx.Context(0)
    finally:
        if old is None:
            del os.environ["VX_TABLE_STREAMS"]
        else:
            os.environ["VX_TABLE_STREAMS"] = old


class HeaderRange:
    def __init__(self, vx, n_headers):
        self.vx, self.ch = vx, vx.synth.Chain(n_headers, profile="Ptiny", stride=512)
        self.sj = vx.synth.Justification(self.ch.target_block, self.ch.target_hash, n_auth=N_AUTH)
        self.just = vx.lib.PackedJustification(self.sj, MAX_AUTH)
        self.args = (16, self.ch.trusted_block, self.ch.trusted_hash, self.ch.target_block)

    def prove(self, ctx, just=None):
        hb = ctx.from_host(self.ch.headers)
        try:
            out, blob = ctx.header_range_prove(hb, 512, self.ch.sizes, *self.args, ctx.stark_config(num_queries=QUERIES), just=just or self.just)
            return out, blob.copy()
        finally:
            hb.free()

    def verify(self, res):
        out, blob = res
        assert out == self.ch.expected_outputs(16)
        self.vx.lib.header_range_verify(blob, *self.args, out, self.vx.lib.default_stark_config(num_queries=QUERIES),
                                        authority_set_hash=self.sj.authority_set_hash, authority_set_id=self.sj.set_id)


class Rotate:
    """The smallest rotation: one new authority, the current set of 4 with 3 signers."""

    def __init__(self, vx):
        self.vx, self.e = vx, vx.synth.EpochEndHeader(150001, 1)
        self.sj = vx.synth.Justification(self.e.number, self.e.hash, n_auth=N_AUTH, n_signed=3, set_id=9)
        self.just = vx.lib.PackedJustification(self.sj, MAX_AUTH)

    def prove(self, ctx):
        e, hb = self.e, ctx.from_host(self.e.padded)
        try:
            out, blob = ctx.rotate_prove(hb, e.size, e.number, 1, e.start_position, e.new_pubkeys, self.just, ctx.stark_config(num_queries=QUERIES))
            return out, blob.copy()
        finally:
            hb.free()

    def verify(self, res):
        out, blob = res
        assert out == self.e.new_authority_set_hash
        self.vx.lib.rotate_verify(blob, 9, self.sj.authority_set_hash, out, self.vx.lib.default_stark_config(num_queries=QUERIES))


@pytest.fixture(scope="module")
def roots(vx):
    """One host context of each kind, alive side by side in this process."""
    cs = {m: make_context(vx, m) for m in MODES}
    yield cs
    for c in cs.values():
        c.close()


@pytest.fixture(scope="module")
def requests_(vx):
    return {"hr1": HeaderRange(vx, 1), "hr2": HeaderRange(vx, 2), "rotate": Rotate(vx)}


@pytest.fixture(scope="module")
def proven(roots, requests_):
    """Every request proven once per mode from ONE host thread (computed on first use, never changed)."""
    cache = {}

    def get(name, mode):
        if (name, mode) not in cache:
            cache[name, mode] = requests_[name].prove(roots[mode])
        return cache[name, mode]

    return get


@pytest.mark.parametrize("name", ["hr1", "hr2", "rotate"])
def test_same_bytes_in_both_modes(requests_, proven, name):
    own, shared = proven(name, "own"), proven(name, "shared")
    assert own[0] == shared[0]
    assert own[1].size == shared[1].size and (own[1] == shared[1]).all(), "the blobs of the two modes differ"
    requests_[name].verify(own)
    requests_[name].verify(shared)


def test_two_shared_contexts_from_two_threads(vx, requests_, proven):
    """Two proofs at once, each with its tables on its own one stream: both verify and equal the single-threaded bytes."""
    req, want = requests_["hr2"], proven("hr2", "shared")
    cs = [make_context(vx, "shared") for _ in range(2)]
    got, errs = [None, None], []

    def worker(i):
        try:
            got[i] = req.prove(cs[i])
        except BaseException as e:  # noqa: BLE001 -- re-raised below
            errs.append(e)

    try:
        ths = [threading.Thread(target=worker, args=(i,)) for i in range(2)]
        for t in ths:
            t.start()
        for t in ths:
            t.join()
    finally:
        for c in cs:
            c.close()
    if errs:
        raise errs[0]
    for res in got:
        req.verify(res)
        assert res[0] == want[0] and (res[1] == want[1]).all()


def test_wrong_authority_set_hash_is_refused_alike(vx, roots, requests_, proven):
    """The commitment table's thread refuses the justification while the other tables wait at the rendezvous: the same code and
    text in both modes, and the context proves the good request afterwards."""
    req = requests_["hr1"]
    bad = vx.lib.PackedJustification(req.sj, MAX_AUTH)
    bad.sh[0] ^= 1
    said = {}
    for mode in MODES:
        with pytest.raises(vx.VxError) as e:
            req.prove(roots[mode], just=bad)
        said[mode] = (e.value.code, str(e.value))
        assert e.value.code == -5 and re.search(r"authority.set commitment mismatch", str(e.value)), str(e.value)
        after = req.prove(roots[mode])
        req.verify(after)
        assert (after[1] == proven("hr1", mode)[1]).all()
    assert said["own"] == said["shared"]


@pytest.mark.parametrize("mode", MODES)
def test_contexts_come_and_go(vx, requests_, mode):
    """A host context, its side contexts made by a proof, all destroyed; three times in a row.  (A shared stream is destroyed once,
    by the context that owns it.)"""
    L = vx.lib.load_library()
    for _ in range(3):
        c = make_context(vx, mode)
        try:
            requests_["hr1"].prove(c)
            c.sync()
        finally:
            h, c.h = c.h, None
            assert L.vx_ctx_destroy(h) == 0
