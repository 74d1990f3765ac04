"""What links two ranks of a series cut into timestep slabs -- the slab pass (dist_kernels.hip behind ftkx_series_dist_begin / _cull /
_serve / _finish) and the host-driven compact halo (halo_kernels.hip behind ftkx_export_masks[_packed], ftkx_push_masked_slice[_packed],
ftkx_sweep_cull, ftkx_get_sparse_cells, ftkx_gather_patches / ftkx_scatter_patches) -- on the meshes of tests/mesh_cases.py: the array lattice
at (5, 7[, 3]), the core strictly inside the domain.  Every other test of these calls has the array at 0 and core = domain, where a dropped
`- m.ext_st[a]`, a core taken for the domain, a summary row divided by the wrong count or a block row not clipped at DH changes nothing.

The reference is the CPU oracle on the case's own mesh (mesh_cases.reference), bit for bit; the premises -- cuts, the bounds L_t <= asked <=
C_t of a request, the cells R_t it must hold, the slabs that must decline, the plain reference of the word compaction, the patch
addresses -- are tests/halo_cases.py's, shown without a GPU in tests/test_halo_cases.py.

A  the slab pass on every case and every cut          C  both exporters against the plain compaction
B  the host-driven halo on the same boundaries        D  the messages ON their limits, damaged headers, the owner alone, the stale flag"""
import contextlib

import numpy as np
import pytest

import halo_cases as H
import mesh_cases as M
import test_gpu_mesh_geometry as G
import test_gpu_slab_inprocess as S
from common import assert_records_equal

pytestmark = pytest.mark.gpu

NAMES = G.NAMES
SUMMARY = G.SUMMARY + ["3d_scalar_40x21x11_huge"]
E_INVALID, E_NOSLICE, E_UNSUPPORTED = -1, -4, -5
MAGIC = 0x66746b786d61736b                                    # "ftkxmask" (halo_kernels.hip: kPackedMagic)
PIPELINED = {("2d_scalar_40x23_ragged", (0, 2, 4)), ("3d_vector_24x13x9_ragged", (0, 1, 2, 3))}      # two passes in flight: one cut per dimension
GUARD = 0x5a5a5a5a5a5a5a5a
FIELDS = ["magic", "summary_bytes", "capacity", "rows", "factor", "count"]


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available()
    import ftk_amd
    from ftk_amd import build
    build.build()
    return ftk_amd


@pytest.fixture(scope="module")
def cases(oracle):
    return M.cases()


@contextlib.contextmanager
def _stream():
    import torch
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    torch.cuda.set_stream(stream)
    try:
        yield torch, dev, stream
    finally:
        torch.cuda.synchronize()
        torch.cuda.set_stream(torch.cuda.default_stream())


def _factory(gpu, c):
    """stream -> a context on the case's mesh, as test_gpu_mesh_geometry._ctx makes it"""
    def make(stream):
        ctx = gpu.Context(c.nd)
        ctx.set_stream(stream.cuda_stream)
        ctx.set_mesh(c.dom, c.core, c.ext)
        ctx.set_options(jacobian_symmetric=int(c.nv == 1), derive_jacobian=1, tag_mode=c.tag_mode)
        return ctx
    return make


def _env(monkeypatch, c, **kw):
    if c.mask_plan:
        monkeypatch.setenv("FTKX_MASK_PLAN", c.mask_plan)
    for k, v in kw.items():
        if v is None:
            monkeypatch.delenv(k, raising=False)
        else:
            monkeypatch.setenv(k, str(v))


def _steps(c):
    return {t: np.array(a) for t, a in c.slices().items()}


def _ranks(gpu, c, cut, torch, dev, stream):
    world = len(cut) - 1
    return [S.Rank(gpu, torch, dev, stream, c.nd, c.nv, c.dims, _steps(c), c.n, world, r, make_ctx=_factory(gpu, c), cut=list(cut)) for r in range(world)]


def _close(ranks):
    for r in ranks:
        if r.ctx is not None:
            r.ctx.close()


# ---- messages ----------------------------------------------------------------------------------------------------------------------------------
def _pad8(v):
    return (v + 7) // 8 * 8


def _parse(buf):
    """a packed mask message (uint8 tensor) -> its header's fields, summary array, word indices and words"""
    b = buf.cpu().numpy()
    n, ub, geo, magic = (int(v) for v in b[:32].copy().view(np.uint64))
    cap, rows, flog = geo & ((1 << 48) - 1), (geo >> 48) & 0xff, geo >> 56
    msg = dict(n=n, ub=ub, cap=cap, rows=rows, flog=flog, magic=magic)
    if magic == MAGIC and 32 + _pad8(ub) + _pad8(cap * 4) + cap * 8 <= len(b):
        k = min(n, cap)
        off_idx = 32 + _pad8(ub)
        off_words = off_idx + _pad8(cap * 4)
        msg["U"] = b[32:32 + ub].copy()
        msg["idx"] = b[off_idx:off_idx + 4 * k].copy().view(np.uint32).astype(np.int64)
        msg["words"] = b[off_words:off_words + 8 * k].copy().view(np.uint64)
    return msg


def _edit_header(torch, buf, field):
    """ONE field of the message's header changed, in device memory"""
    h = buf[:32].cpu().numpy().copy().view(np.uint64)
    n, ub, geo = int(h[0]), int(h[1]), int(h[2])
    cap, rows, flog = geo & ((1 << 48) - 1), (geo >> 48) & 0xff, geo >> 56
    assert int(h[3]) == MAGIC and n <= cap, "a good message to begin with"
    if field == "magic":
        h[3] = MAGIC ^ 1
    elif field == "summary_bytes":
        h[1] = ub + 8
    elif field == "capacity":
        cap += 1
    elif field == "rows":
        rows = 1 if rows != 1 else 4
    elif field == "factor":
        flog += 1                                             # (the receiver is told the sender's own factor: one above it)
    elif field == "count":
        h[0] = cap + 1
    else:
        raise ValueError(field)
    h[2] = cap | (rows << 48) | (flog << 56)
    buf[:32].copy_(torch.from_numpy(h.view(np.uint8)).to(buf.device))


def _check_message(c, U, idx, words, n, u_rows, what):
    """count and sorted index list are those of the plain compaction of the message's own summary array; no index repeats -> index -> word"""
    ngroups, UP, P, urows, DH, DD = H.summary_layout(c.dims, u_rows)
    assert len(U) == UP * urows * DD, (what, len(U), UP, urows, DD)
    want = H.compacted(U, c.dims, u_rows)
    assert n == len(want) == len(idx), (what, n, len(want), len(idx))
    order = np.argsort(idx, kind="stable")
    assert len(np.unique(idx)) == len(idx), f"{what}: an index repeats"
    assert np.array_equal(idx[order], want), f"{what}: the word list is not the one its summary array implies"
    return idx[order], np.asarray(words)[order]


def _u_rows(c, env):
    family, summaries, rows = M.planned(c, env, rows=True)
    assert summaries
    return rows


def _same_masks(a, b, what):
    """two messages of one slice under one factor: the same summary array, the same words at the same places"""
    assert np.array_equal(a[0], b[0]), f"{what}: summary arrays differ"
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), f"{what}: word lists differ"


# ---- the reference -------------------------------------------------------------------------------------------------------------------------------
def _assert_steps(recs, c, lo, hi, what):
    """the records of the steps lo .. hi - 1 equal the reference's, bit for bit and in tag order"""
    ref, _, _ = M.reference(c)
    ref = ref[(ref["timestep"] >= lo) & (ref["timestep"] < hi)]
    assert len(recs) == len(ref) > 0, f"{what}: {len(recs)} records, expected {len(ref)}"
    assert np.array_equal(recs["tag"], ref["tag"]), f"{what}: tags differ or are out of order"
    assert_records_equal(G._as_fixture(recs), ref, coord_tol=0.0, what=what)


def _assert_request(c, t, cells, what):
    """the three conditions a request for the slice behind step t keeps"""
    L, Cc, R = H.request_bounds(c, t)
    cells = np.asarray(cells, dtype=np.int64)
    print(what, "asked", len(cells), "L_t", L, "C_t", Cc, "R_t", len(R))
    assert L <= len(cells) <= Cc, (what, L, len(cells), Cc)
    assert len(np.unique(cells)) == len(cells), f"{what}: a cell is asked for twice"
    assert cells.min() >= 0 and cells.max() < c.cells, (what, int(cells.min()), int(cells.max()), c.cells)
    assert np.isin(R, cells).all(), f"{what}: {int((~np.isin(R, cells)).sum())} cells with an interval record are not in the request"


# ---- the slab pass -----------------------------------------------------------------------------------------------------------------------------
def _slab_run(gpu, c, cut, *, pipelined=False, tamper=None, refused=(), what=""):
    """one slab pass (two in flight: pipelined) of the case under the cut, completed, merged and compared with the reference.  refused: ranks
    that must ask -1 although their slab does not decline (a limit or a damaged message).  -> {rank: dict(asked, cells, masks_out)}"""
    world = len(cut) - 1
    info = {}
    with _stream() as (torch, dev, stream):
        ranks = _ranks(gpu, c, cut, torch, dev, stream)
        try:
            # the request and the mask message lie in front of guard words: a cell stored at slot `cap`, a word stored at `capacity`, shows
            guards = []
            for r in ranks:
                for key, dtype, fill in (("req_out", torch.int64, GUARD), ("masks_out", torch.uint8, GUARD & 0xff)):
                    n = r.sets[0][key].numel()
                    big = torch.full((n + 64,), fill, dtype=dtype, device=dev)
                    big[:n].zero_()
                    r.sets[0][key] = big[:n]
                    guards.append((r.rank, key, big, n, fill))
            S._slab_pass(ranks, 0, tamper=tamper)
            if pipelined:
                S._slab_pass(ranks, 1)
            results, recovered = S._complete(ranks)
            for rank, key, big, n, fill in guards:
                assert bool((big[n:] == fill).all()), (what, cut, rank, f"something was stored behind the end of {key}")
            for r in ranks:
                decline = H.must_decline(c, cut, r.rank)
                path, status = r.ctx.series_last_path()
                i = info[r.rank] = dict(asked=None, path=path, status=status)
                if r.lower is not None:
                    i["masks_out"] = _parse(r.sets[0]["masks_out"])
                if r.upper is not None:
                    req = r.sets[0]["req_out"].cpu().numpy()
                    i["asked"] = int(req[0])
                    i["cells"] = req[1:1 + max(0, int(req[0]))].copy()
                    t = r.own[-1]
                    if decline or r.rank in refused:
                        assert i["asked"] == -1, (what, cut, r.rank, i["asked"], "this rank had to ask for the whole slice")
                    else:
                        assert i["asked"] >= 0, (what, cut, r.rank, i, "this rank had no reason to ask for the whole slice")
                        _assert_request(c, t, i["cells"], f"{what} {cut} rank {r.rank}")
                if not decline and r.rank not in refused:
                    assert path in (1, 2, 5) and not (status & G.NOT_DEVICE_DRIVEN), (what, cut, r.rank, path, status, "a device-driven form was due")
                elif decline and r.upper is None:
                    assert path == 0 and (status & G.NOT_DEVICE_DRIVEN) == G.MASKS_INVALID, (what, cut, r.rank, path, status)
            expected = sum(1 for r in ranks if r.upper is not None and (H.must_decline(c, cut, r.rank) or r.rank in refused))
            assert recovered == expected, (what, cut, recovered, expected)
            if pipelined:
                results2, _ = S._complete(ranks)
                for (r, a), (r2, b) in zip(results, results2):
                    assert a[1] == b[1] and a[0].tobytes() == b[0].tobytes(), (what, cut, "the second pass in flight differs from the first")
            merged = np.concatenate([res[0] for _, res in results])
            merged = merged[np.argsort(merged["tag"], kind="stable")]
            factors = {}
            for r, res in results:
                for t, f in zip(r.own, res[1]):
                    factors[t] = f
            G._assert_reference(merged, [factors[t] for t in range(c.n)], c, f"{what} {cut}")
            for r, res in results:
                _assert_steps(res[0][np.argsort(res[0]["tag"], kind="stable")], c, r.own[0], r.own[-1] + 1, f"{what} {cut} rank {r.rank}")
        finally:
            _close(ranks)
    return info


@pytest.mark.parametrize("name", NAMES)
def test_slab_pass_on_every_cut(gpu, cases, name, monkeypatch):
    """A.  FTKX_DIST_CELLS = C_t: a request can hold every cell, so that the compact way is the one taken wherever no decline is due"""
    c = cases[name]
    _env(monkeypatch, c, FTKX_DIST_CELLS=c.cells)
    for cut in H.cuts(c):
        if not c.summaries:
            # a mesh without summarised masks: every rank says so alike at _begin, and nothing stays half queued
            with _stream() as (torch, dev, stream):
                ranks = _ranks(gpu, c, cut, torch, dev, stream)
                try:
                    for r in ranks:
                        b = r.sets[0]
                        with pytest.raises(gpu.FtkxError) as e:
                            r.ctx.series_dist_begin(r.ts, r.scopes, None, r.rank, r.world, r.upper, b["contrib"], b["gathered"], b["masks_out"] if r.lower is not None else None)
                        assert e.value.code == E_UNSUPPORTED, (name, cut, r.rank, e.value)
                        # (ftkx_sweep_series refuses a context with a slab pass half queued)
                        recs, f, _ = r.ctx.sweep_series(r.ts, [gpu.SCOPE_ORDINAL] * len(r.ts))
                        assert len(recs) > 0
                finally:
                    _close(ranks)
            continue
        info = _slab_run(gpu, c, cut, pipelined=(name, cut) in PIPELINED, what=name)
        for rank, i in info.items():
            # C: the slab pass's own export against the plain compaction
            if "masks_out" in i and not H.must_decline(c, cut, rank):
                m = i["masks_out"]
                assert m["magic"] == MAGIC and m["rows"] == _u_rows(c, None), (name, cut, rank, m["rows"])
                _check_message(c, m["U"], m["idx"], m["words"], m["n"], m["rows"], f"{name} {cut} rank {rank} masks_out")


# ---- the host-driven compact halo -------------------------------------------------------------------------------------------------------------
class Pair:
    """two contexts on one GPU: A holds the slices lo .. b - 1, B -- the owner -- the slice b; both prepared under the hint 256"""

    def __init__(self, gpu, c, lo, b, torch, dev, stream):
        self.gpu, self.c, self.lo, self.b, self.torch, self.dev = gpu, c, lo, b, torch, dev
        self.scalar = c.nv == 1
        self.own = list(range(lo, b))
        self.factors = [M.reference(c)[1][c.ts.index(t)] for t in self.own]
        make = _factory(gpu, c)
        self.A, self.B = make(stream), make(stream)
        for t in self.own:
            self.push(self.A, t)
        self.push(self.B, b)
        self.A.slices_prepare(self.own, 0)
        self.rmB = self.B.slices_prepare([b], 0)
        self.nbytes, self.cap = self.B.packed_masks_bytes()

    def push(self, ctx, t):
        (ctx.push_scalar_slice if self.scalar else ctx.push_slice)(t, self.c.slices()[t])

    def export(self, form):
        """the owner's message: ("packed", the uint8 tensor) or ("lists", (U, idx, words, factor, max))"""
        if form == "packed":
            buf = self.torch.zeros((self.nbytes,), dtype=self.torch.uint8, device=self.dev)
            self.B.export_masks_packed(self.b, buf)
            return buf
        return self.B.export_masks(self.b, self.torch, self.dev)

    def deliver(self, form, msg):
        if form == "packed":
            self.A.push_masked_slice_packed(self.b, self.scalar, msg, 256, self.rmB[self.b][1])
        else:
            U, idx, words, mf, mx = msg
            self.A.push_masked_slice(self.b, self.scalar, U, idx, words, mf, mx)

    def enqueue(self):
        self.A.sweep_enqueue_many(self.own, [self.gpu.SCOPE_BOTH] * len(self.own), self.factors)

    def cull(self):
        return self.A.sweep_cull(self.b, self.torch, self.dev)

    def finish(self, cells, what):
        """the cells checked, their patches gathered on the owner, checked and scattered, the batch collected and compared"""
        c = self.c
        _assert_request(c, self.b - 1, cells.cpu().numpy(), what)
        ncomp = 1 if self.scalar else c.nd
        got = self.B.gather_patches(self.b, cells, self.torch)
        flat = c.slices()[self.b].reshape(-1, ncomp)
        want = flat[H.patch_addresses(c, cells.cpu().numpy())]
        assert np.array_equal(got.cpu().numpy().reshape(len(cells), 6 ** c.nd, ncomp), want), f"{what}: gathered patches are not the array's values at cell - ext_st"
        self.A.scatter_patches(self.b, cells, got)
        _assert_steps(np.array(self.A.sweep_collect()), c, self.lo, self.b, what)

    def recover(self, what):
        """the protocol's answer to a refusal: cancel, the slice itself, the same steps again"""
        self.A.sweep_cancel()
        self.push(self.A, self.b)
        self.enqueue()
        _assert_steps(np.array(self.A.sweep_collect()), self.c, self.lo, self.b, what + " [recovered]")

    def enqueue_with_the_slice(self, what):
        """no masks to hand over: the slice itself, the steps, the reference"""
        self.push(self.A, self.b)
        self.enqueue()
        _assert_steps(np.array(self.A.sweep_collect()), self.c, self.lo, self.b, what + " [the slice itself]")

    def close(self):
        self.A.close(); self.B.close()


def _boundaries(c):
    """(lower slab's first step, halo slice, cut, lower rank) of every boundary of every cut, each pair of slabs once"""
    seen, out = set(), []
    for cut in H.cuts(c):
        for r, t in H.boundaries(cut):
            if (cut[r], t + 1) not in seen:
                seen.add((cut[r], t + 1))
                out.append((cut[r], t + 1, cut, r))
    return out


@pytest.mark.parametrize("rows", [None, "1", "4"])
@pytest.mark.parametrize("name", SUMMARY)
def test_host_driven_halo_on_every_boundary(gpu, cases, name, rows, monkeypatch):
    """B, and C for the two host-driven exporters.  FTKX_U_ROWS: the default, 1, and 4 in 3D"""
    c = cases[name]
    if rows == "4" and c.nd == 2:
        return                                                # (2D block summaries are four rows by default: nothing else to select)
    _env(monkeypatch, c, FTKX_U_ROWS=rows)
    u_rows = _u_rows(c, rows)
    for lo, b, cut, rank in _boundaries(c):
        decline = H.must_decline(c, cut, rank)
        exported = {}
        for form in ("lists", "packed"):
            what = f"{name} [{lo}, {b}) <- {b} {form} FTKX_U_ROWS={rows}"
            with _stream() as (torch, dev, stream):
                p = Pair(gpu, c, lo, b, torch, dev, stream)
                try:
                    if c.kind == "huge":
                        # every vertex may wrap a determinant: ftkx_slices_prepare builds no masks, the owner has none to export and says so;
                        # the slice itself goes over
                        with pytest.raises(gpu.FtkxError) as e:
                            p.export(form)
                        assert decline and e.value.code == E_UNSUPPORTED, (what, e.value)
                        p.enqueue_with_the_slice(what)
                        exported[form] = (8, (None, None, None))
                        continue
                    msg = p.export(form)
                    if form == "packed":
                        m = _parse(msg)
                        assert m["magic"] == MAGIC and m["rows"] == u_rows and m["cap"] == p.cap and m["ub"] == len(m["U"]), (what, m["rows"], u_rows)
                        exported[form] = (m["flog"], (m["U"],) + _check_message(c, m["U"], m["idx"], m["words"], m["n"], u_rows, what))
                    else:
                        U, idx, words, mf, mx = msg
                        Un, idxn, wn = U.cpu().numpy(), idx.cpu().numpy().view(np.uint32).astype(np.int64), words.cpu().numpy().view(np.uint64)
                        assert mf == 256 and mx == p.rmB[b][1]
                        exported[form] = (8, (Un,) + _check_message(c, Un, idxn, wn, len(idxn), u_rows, what))
                    p.deliver(form, msg)
                    p.enqueue()
                    try:
                        cells = p.cull()
                    except gpu.FtkxError as e:
                        # masks without the per-vertex rule do not serve a factor under which a determinant could wrap
                        assert decline and e.code in (E_NOSLICE, E_UNSUPPORTED), (what, e)
                        p.recover(what)
                        continue
                    p.finish(cells, what)
                finally:
                    p.close()
        assert exported["lists"][0] == exported["packed"][0] == 8
        if c.kind != "huge":
            _same_masks(exported["lists"][1], exported["packed"][1], f"{name} slice {b}: export_masks and export_masks_packed")


# ---- both exporters of one slice ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SUMMARY)
def test_the_exporters_agree(gpu, cases, name, monkeypatch):
    """C.  compact_words_kernel takes one lane per word, dist_export_kernel eight summary bytes per lane: under one factor they describe
    one slice alike -- the same summary array, the same indices, the same words"""
    c = cases[name]
    _env(monkeypatch, c, FTKX_DIST_CELLS=c.cells)
    u_rows = _u_rows(c, None)
    compared = 0
    for cut in [k for k in H.cuts(c) if len(k) == 3]:
        if H.must_decline(c, cut, 1):
            continue                                          # (the owner's pass declines: its masks are not ones to compare)
        b = cut[1]
        m = _slab_run(gpu, c, cut, what=name)[1]["masks_out"]
        assert m["magic"] == MAGIC and m["rows"] == u_rows
        slab = (m["U"],) + _check_message(c, m["U"], m["idx"], m["words"], m["n"], u_rows, f"{name} {cut} masks_out")
        with _stream() as (torch, dev, stream):
            p = Pair(gpu, c, max(0, b - 1), b, torch, dev, stream)
            try:
                h = _parse(p.export("packed"))
            finally:
                p.close()
        host = (h["U"],) + _check_message(c, h["U"], h["idx"], h["words"], h["n"], u_rows, f"{name} slice {b} export_masks_packed")
        print(name, cut, "factor bytes", m["flog"], h["flog"], "words", m["n"], h["n"])
        if m["flog"] == h["flog"]:
            _same_masks(slab, host, f"{name} slice {b}: dist_export_kernel and compact_words_kernel")
            compared += 1
    if not any(H.must_decline(c, cut, 1) for cut in H.cuts(c) if len(cut) == 3):
        assert compared >= 1, (name, "no pair of messages under one factor")


# ---- D: the limits -----------------------------------------------------------------------------------------------------------------------------
def _limit(cases, k):
    name, cut, t = H.LIMIT_CASES[k]
    c = cases[name]
    r = [r for r, tb in H.boundaries(cut) if tb == t][0]
    return c, cut, t, r


def _packed_run(gpu, c, lo, b, what, *, damage=None, receiver_env=None, monkeypatch=None, refused=False):
    """export_masks_packed -> (damage) -> push_masked_slice_packed -> enqueue -> sweep_cull: succeeds and gives the reference, or -- refused --
    raises FTKX_E_NOSLICE and the protocol's answer gives the reference.  -> the message's word count"""
    with _stream() as (torch, dev, stream):
        p = Pair(gpu, c, lo, b, torch, dev, stream)
        try:
            buf = torch.zeros((max(p.nbytes, 1 << 17),), dtype=torch.uint8, device=dev)
            p.B.export_masks_packed(b, buf)
            n = _parse(buf)["n"]
            if damage:
                _edit_header(torch, buf, damage)
            if receiver_env:
                monkeypatch.setenv(*receiver_env)
            p.deliver("packed", buf)
            p.enqueue()
            if refused:
                with pytest.raises(gpu.FtkxError) as e:
                    p.cull()
                assert e.value.code == E_NOSLICE, (what, e.value)
                p.recover(what)
            else:
                p.finish(p.cull(), what)
        finally:
            p.close()
    return n


def test_word_list_exactly_full_and_one_short(gpu, cases, monkeypatch):
    """D.1  FTKX_HALO_WORDS = the count a run at the default capacity gives: the message fits; one less: both receivers refuse it"""
    counts = []
    for k in range(len(H.LIMIT_CASES)):
        c, cut, t, r = _limit(cases, k)
        _env(monkeypatch, c, FTKX_DIST_CELLS=c.cells, FTKX_HALO_WORDS=None)
        what = f"{c.name} {cut} t {t}"
        n = _packed_run(gpu, c, cut[r], t + 1, what + " [packed, default capacity]")
        n_slab = _slab_run(gpu, c, cut, what=what)[r + 1]["masks_out"]["n"]
        print(what, "words: packed", n, "slab", n_slab)
        counts += [n, n_slab]
        assert n >= 2 and n_slab >= 2
        monkeypatch.setenv("FTKX_HALO_WORDS", str(n))
        assert _packed_run(gpu, c, cut[r], t + 1, what + " [packed, capacity = count]") == n
        monkeypatch.setenv("FTKX_HALO_WORDS", str(n - 1))
        assert _packed_run(gpu, c, cut[r], t + 1, what + " [packed, capacity = count - 1]", refused=True) == n
        monkeypatch.setenv("FTKX_HALO_WORDS", str(n_slab))
        info = _slab_run(gpu, c, cut, what=what + " [capacity = count]")
        assert info[r + 1]["masks_out"]["n"] == info[r + 1]["masks_out"]["cap"] == n_slab and info[r]["asked"] >= 0
        monkeypatch.setenv("FTKX_HALO_WORDS", str(n_slab - 1))
        info = _slab_run(gpu, c, cut, refused={r}, what=what + " [capacity = count - 1]")
        assert info[r + 1]["masks_out"]["n"] == n_slab == info[r + 1]["masks_out"]["cap"] + 1 and info[r]["asked"] == -1
    assert any(n > 64 and n % 64 != 0 for n in counts), counts            # a wavefront's reservation that ends inside a wavefront


def test_request_exactly_full_and_one_short(gpu, cases, monkeypatch):
    """D.2  FTKX_DIST_CELLS = the count a roomy request gives: asked == served == n, the compact way; one less: -1 on both sides"""
    for k in range(len(H.LIMIT_CASES)):
        c, cut, t, r = _limit(cases, k)
        _env(monkeypatch, c, FTKX_DIST_CELLS=c.cells)
        what = f"{c.name} {cut} t {t}"
        n = _slab_run(gpu, c, cut, what=what)[r]["asked"]
        assert n >= 65 and n >= H.request_bounds(c, t)[0]
        monkeypatch.setenv("FTKX_DIST_CELLS", str(n))
        info = _slab_run(gpu, c, cut, what=what + " [request = count]")          # (asked == served is asserted by _complete)
        assert info[r]["asked"] == n
        monkeypatch.setenv("FTKX_DIST_CELLS", str(n - 1))
        info = _slab_run(gpu, c, cut, refused={r}, what=what + " [request = count - 1]")
        assert info[r]["asked"] == -1


@pytest.mark.parametrize("field", FIELDS + ["receiver_capacity"])
def test_damaged_headers_are_refused(gpu, cases, field, monkeypatch):
    """D.3  ONE field of a good message's header changed in device memory (or a receiver whose FTKX_HALO_WORDS is not the sender's): the
    packed receiver refuses through ftkx_sweep_cull, the slab receiver asks -1; the recovery gives the reference.  Every such message is
    turned away before any store (no word index outside the mask array is ever sent: a broken guard there would be a wild store)"""
    for k in range(len(H.LIMIT_CASES)):
        c, cut, t, r = _limit(cases, k)
        _env(monkeypatch, c, FTKX_DIST_CELLS=c.cells, FTKX_HALO_WORDS=None)
        what = f"{c.name} {cut} t {t} [{field}]"
        if field == "receiver_capacity":
            _packed_run(gpu, c, cut[r], t + 1, what, receiver_env=("FTKX_HALO_WORDS", "4000"), monkeypatch=monkeypatch, refused=True)
            monkeypatch.delenv("FTKX_HALO_WORDS")
            _slab_run(gpu, c, cut, refused={r}, what=what, tamper=lambda ranks, kk: monkeypatch.setenv("FTKX_HALO_WORDS", "4000"))
            monkeypatch.delenv("FTKX_HALO_WORDS")
        else:
            _packed_run(gpu, c, cut[r], t + 1, what, damage=field, refused=True)
            _slab_run(gpu, c, cut, refused={r}, what=what, tamper=lambda ranks, kk: _edit_header(ranks[r].torch, ranks[r].sets[kk]["masks_in"], field))


def test_the_owner_alone(gpu, cases, monkeypatch):
    """D.4  ftkx_series_dist_serve with hand-made requests into a reply pre-filled with a sentinel: a count of 0, -1 or cap + 1 leaves the
    reply untouched and `served` reports the word; valid cells get the array's values at their patch addresses, a cell index beyond the
    core's cells a patch of zeros, nothing behind the last patch is written.  The pass is then finished and completed (`served` is read from
    the completed pass), and one more is aborted behind _serve: the context sweeps on"""
    SENTINEL = -12345.0
    for k in range(len(H.LIMIT_CASES)):
        c, cut, t, r = _limit(cases, k)
        cap = 96
        _env(monkeypatch, c, FTKX_DIST_CELLS=cap)
        ncomp, pe = (1 if c.nv == 1 else c.nd), 6 ** c.nd
        flat = c.slices()[t + 1].reshape(-1, ncomp)
        rng = np.random.default_rng(17)
        valid = np.unique(np.concatenate([[0, c.core[1][0] - 1, c.core[1][0], c.cells - 1], rng.integers(0, c.cells, size=70)]))
        foreign_at = 37
        cells = np.concatenate([valid[:foreign_at], [c.cells], valid[foreign_at:], [c.cells + 12345]]).astype(np.int64)
        assert 64 < len(cells) <= cap
        with _stream() as (torch, dev, stream):
            ranks = _ranks(gpu, c, cut, torch, dev, stream)
            try:
                o = ranks[r + 1]
                b = o.sets[0]
                assert o.ctx.series_dist_cells() == cap and b["reply_out"].numel() == cap * pe * ncomp
                neutral = torch.tensor([S.DBL_MAX, 0.0, S.DBL_MAX, 0.0] * o.world, dtype=torch.float64, device=dev)

                def serve(request, finish):
                    b["gathered"].copy_(neutral)
                    b["req_in"].zero_()
                    b["req_in"][:len(request)].copy_(torch.from_numpy(np.asarray(request, dtype=np.int64)).to(dev))
                    b["reply_out"].fill_(SENTINEL)
                    o.ctx.series_dist_begin(o.ts, o.scopes, None, o.rank, o.world, o.upper, b["contrib"], b["gathered"], b["masks_out"])
                    o.ctx.series_dist_cull(None, None)
                    o.ctx.series_dist_serve(b["req_in"], b["reply_out"])
                    if not finish:
                        o.ctx.sweep_series_abort()
                        return None, b["reply_out"].cpu().numpy()
                    o.ctx.series_dist_finish(None)
                    o.ctx.sweep_series_complete(copy=True)
                    return o.ctx.series_dist_status(o.world)[1], b["reply_out"].cpu().numpy()
                assert o.upper is None, "the owner of the limit boundaries is the last rank: no halo of its own"
                for word in (0, -1, cap + 1):
                    served, reply = serve([word] + list(cells[:5]), True)
                    assert served == word and (reply == SENTINEL).all(), (c.name, word, served)
                served, reply = serve([len(cells)] + list(cells), True)
                assert served == len(cells)
                got = reply[:len(cells) * pe * ncomp].reshape(len(cells), pe, ncomp)
                inside = cells < c.cells
                assert np.array_equal(got[inside], flat[H.patch_addresses(c, cells[inside])]), f"{c.name}: served patches are not the array's values at cell - ext_st"
                assert int((~inside).sum()) == 2 and not got[~inside].any(), f"{c.name}: a cell outside the core got values"
                assert (reply[len(cells) * pe * ncomp:] == SENTINEL).all()
                # aborted behind _serve: nothing stays half queued, the next pass runs
                _, reply = serve([3] + list(valid[:3]), False)
                assert np.array_equal(reply[:3 * pe * ncomp].reshape(3, pe, ncomp), flat[H.patch_addresses(c, valid[:3])])
                served, _ = serve([0], True)
                assert served == 0
            finally:
                _close(ranks)


@pytest.mark.parametrize("drop", [False, True])
def test_a_refused_packed_message_does_not_outlive_a_good_one(gpu, cases, drop, monkeypatch):
    """D.5  a refused packed message raises the flag ftkx_sweep_cull looks at; a good message for the same slice, pushed with no cull in
    between (drop: behind ftkx_drop_slice), replaces its masks and must take the flag down: the cull succeeds and gives the reference"""
    for k in range(len(H.LIMIT_CASES)):
        c, cut, t, r = _limit(cases, k)
        _env(monkeypatch, c)
        what = f"{c.name} {cut} t {t} drop {drop}"
        with _stream() as (torch, dev, stream):
            p = Pair(gpu, c, cut[r], t + 1, torch, dev, stream)
            try:
                good = p.export("packed")
                bad = good.clone()
                _edit_header(torch, bad, "magic")
                p.deliver("packed", bad)
                if drop:
                    p.A.drop_slice(t + 1)
                p.deliver("packed", good)
                p.enqueue()
                p.finish(p.cull(), what)
            finally:
                p.close()
