"""CPU tier: the guard-band helper (tests/guarded_alloc.py) on host tensors, through its ``guard_cpu`` flag: a one-byte write just
before or just after a buffer is reported with the buffer's name, side and offset; writing the whole interior is not; views come out
aligned, typed, shaped and contiguous; the ``torch`` proxy leaves host and pinned allocations alone; ``covers`` / ``handed_out``
answer as documented.  (The GPU tiers, test_gpu_bounds_*.py, rely on exactly these properties.)"""
import re
import types

import pytest
import torch

import guarded_alloc
from guarded_alloc import ALIGN, FILLS, GUARD_BYTES, Guards, TorchProxy


def _raw(g, i=-1):
    b = g.live[i]
    return b.raw, b.off, b.nbytes


@pytest.mark.parametrize("fill", FILLS)
def test_clean_when_the_whole_interior_is_written(fill):
    g = Guards(fill, guard_cpu=True)
    for shape, dtype in [((7, 3), torch.float32), ((1001,), torch.uint8), ((5, 2, 3), torch.int64), ((), torch.float32), ((0, 4), torch.float32)]:
        t = g.guarded(shape, dtype, "cpu", "buf")
        raw, off, n = _raw(g)
        raw[off:off + n] = 0x5A                      # every byte of the interior, and none outside
        assert t.numel() == 0 or t.view(-1).view(torch.uint8)[-1] == 0x5A
    g.check()
    assert g.checked == 5 and not g.live


@pytest.mark.parametrize("fill", FILLS)
def test_one_byte_before_is_reported(fill):
    g = Guards(fill, guard_cpu=True)
    g.guarded((4, 4), torch.float32, "cpu", "innocent")
    g.guarded((33,), torch.float32, "cpu", "victim")
    raw, off, n = _raw(g)
    raw[off - 1] = 0x5A
    with pytest.raises(AssertionError) as e:
        g.check()
    msg = str(e.value)
    assert "front guard of 'victim' (132 bytes)" in msg and "first at -1, last at -1" in msg
    assert "innocent" not in msg and "rear" not in msg
    assert not g.live                                 # released even when dirty


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("nbytes", [1, 7, 1003, 513])
def test_one_byte_after_an_odd_sized_buffer_is_reported(fill, nbytes):
    """sizes that are no multiple of 4, 8 or 512: the rear guard starts at the exact next byte"""
    g = Guards(fill, guard_cpu=True)
    t = g.guarded((nbytes,), torch.uint8, "cpu", "odd")
    raw, off, n = _raw(g)
    assert n == nbytes and raw.data_ptr() + off == t.data_ptr()
    raw[off + n] = 0x5A
    with pytest.raises(AssertionError) as e:
        g.check()
    msg = str(e.value)
    assert "rear guard of 'odd' (%d bytes)" % nbytes in msg and "first at +0, last at +0" in msg and "front" not in msg


@pytest.mark.parametrize("fill", FILLS)
def test_both_ends_of_both_guards_are_compared(fill):
    """the first byte of the front guard, the last byte of the rear guard, and a run in between: first and last offsets"""
    for where in ("front0", "rearlast", "run"):
        g = Guards(fill, guard_cpu=True)
        g.guarded((10,), torch.int16, "cpu", "b")
        raw, off, n = _raw(g)
        if where == "front0":
            raw[0] = 0x5A
            want = "front guard of 'b' (20 bytes) dirty: 1 byte(s), first at %+d, last at %+d" % (-off, -off)
        elif where == "rearlast":
            raw[off + n + GUARD_BYTES - 1] = 0x5A
            want = "rear guard of 'b' (20 bytes) dirty: 1 byte(s), first at %+d, last at %+d" % (GUARD_BYTES - 1, GUARD_BYTES - 1)
        else:
            raw[off + n + 4:off + n + 12] = 0x5A
            want = "rear guard of 'b' (20 bytes) dirty: 8 byte(s), first at +4, last at +11"
        with pytest.raises(AssertionError) as e:
            g.check()
        assert want in str(e.value), (where, str(e.value))


def test_a_bit_flip_counts():
    """bit for bit: one flipped bit of one guard byte is a mismatch under either fill"""
    for fill in FILLS:
        g = Guards(fill, guard_cpu=True)
        g.guarded((3,), torch.float64, "cpu", "b")
        raw, off, n = _raw(g)
        raw[off + n + 100] = fill ^ 0x01
        with pytest.raises(AssertionError):
            g.check()


@pytest.mark.parametrize("fill", FILLS)
def test_views(fill):
    g = Guards(fill, guard_cpu=True)
    for shape, dtype in [((3, 5, 7), torch.float32), ((9,), torch.bfloat16), ((2, 2), torch.int64), ((1001,), torch.uint8),
                         ((4, 3), torch.float64), ((6,), torch.int32), ((5, 5), torch.float16)]:
        t = g.guarded(shape, dtype, "cpu")
        raw, off, n = _raw(g)
        assert t.shape == shape and t.dtype == dtype and t.is_contiguous() and t.device.type == "cpu"
        assert t.data_ptr() % ALIGN == 0 and off >= GUARD_BYTES
        assert n == t.numel() * t.element_size()
        assert raw.numel() >= off + n + GUARD_BYTES
        assert (t.view(-1).view(torch.uint8) == fill).all()                # an `empty` interior holds the fill
        assert g.live[-1].name.startswith("test_guarded_alloc.py:") and g.live[-1].name.endswith(" test_views")   # the call site
    src = torch.arange(12, dtype=torch.float32).reshape(3, 4).t()          # not contiguous
    c = g.guarded_copy(src, "copy")
    assert torch.equal(c, src) and c.is_contiguous() and c.data_ptr() % ALIGN == 0 and g.live[-1].name == "copy"
    if fill == 0xFF:
        assert torch.isnan(g.guarded((4,), torch.float32, "cpu")).all() and (g.guarded((4,), torch.int32, "cpu") == -1).all()
    g.check()


def test_proxy_routes_constructors_and_passes_the_rest_through():
    g = Guards(0xFF, guard_cpu=True)
    p = TorchProxy(g)
    assert p.float32 is torch.float32 and p.Tensor is torch.Tensor and p.cat is torch.cat and p.cuda is torch.cuda
    made = [p.empty(3, 4, dtype=torch.int32, device="cpu"), p.empty((3, 4), dtype=torch.int32, device="cpu"), p.zeros(5, device="cpu"),
            p.zeros((), device="cpu"), p.ones((2, 3), dtype=torch.float64, device="cpu"), p.full((4,), -1, dtype=torch.int32, device="cpu"),
            p.full((3,), float("inf"), device="cpu")]
    assert made[0].shape == (3, 4) and made[1].shape == (3, 4) and made[0].dtype == torch.int32
    assert torch.equal(made[2], torch.zeros(5)) and made[3].shape == () and made[3] == 0
    assert torch.equal(made[4], torch.ones(2, 3, dtype=torch.float64)) and torch.equal(made[5], torch.full((4,), -1, dtype=torch.int32))
    assert torch.equal(made[6], torch.full((3,), float("inf"))) and made[6].dtype == torch.float32
    x = torch.arange(6, dtype=torch.int64).reshape(2, 3)
    likes = [p.empty_like(x), p.zeros_like(x), p.ones_like(x), p.full_like(x, 7)]
    assert all(t.shape == x.shape and t.dtype == torch.int64 for t in likes)
    assert torch.equal(likes[1], torch.zeros_like(x)) and torch.equal(likes[2], torch.ones_like(x)) and torch.equal(likes[3], torch.full_like(x, 7))
    assert all(g.covers(t) for t in made + likes) and len(g.live) == len(made) + len(likes)
    assert all(n.startswith("test_guarded_alloc.py:") for n in g.names())
    g.check()
    # without the flag the host is torch's own business, and so is pinned memory with it
    h = Guards(0x00)
    q = TorchProxy(h)
    a, b, c = q.empty(5), q.zeros(3, 3, dtype=torch.float32, device="cpu"), q.full_like(x, 2)
    assert not h.live and not h.covers(a) and not h.covers(b) and not h.covers(c)
    assert b.shape == (3, 3) and torch.equal(c, torch.full_like(x, 2))
    assert not Guards(0x00, guard_cpu=True).wants("cpu", pin_memory=True) and Guards(0x00).wants("cuda:0") and Guards(0x00).wants(torch.device("cuda", 1))
    assert not Guards(0x00).wants(None) and not Guards(0x00).wants("cpu")
    with pytest.raises(AttributeError):
        q.float32 = None


def test_patched_swaps_the_modules_torch_and_restores_it():
    mod = types.ModuleType("fake_wrapper")
    mod.torch = torch
    exec("def make(n):\n    return torch.empty(n, dtype=torch.uint8, device='cpu'), torch.cat([torch.zeros(2, device='cpu')])", mod.__dict__)
    g = Guards(0xFF, guard_cpu=True)
    with g.patched(modules=[mod], package=None):
        assert isinstance(mod.torch, TorchProxy)
        ws, other = mod.make(1003)
    assert mod.torch is torch
    assert g.covers(ws) and g.handed_out(1003) and not g.handed_out(1004) and not g.covers(other)
    with pytest.raises(RuntimeError):
        with g.patched(modules=[mod], package=None):
            raise RuntimeError("inside")
    assert mod.torch is torch
    g.check()
    assert g.handed_out(1003)                          # the ledger outlives check()
    # the real modules all hold a module-level torch for the proxy to stand in for
    import importlib
    for m in guarded_alloc.MODULES:
        assert importlib.import_module("sylber_amd." + m).torch is torch


def test_covers_and_handed_out():
    g = Guards(0x00, guard_cpu=True)
    t = g.guarded((6, 8), torch.float32, "cpu", "t")
    assert g.covers(t) and g.covers(t[2:4]) and g.covers(t[:, 3]) and g.covers(t.view(-1)[47:])
    assert not g.covers(torch.empty(6, 8)) and not g.covers(t.clone()) and not g.covers(None)
    raw, off, n = _raw(g)
    assert not g.covers(raw) and not g.covers(raw[off - 1:off + n]) and not g.covers(raw[off:off + n + 1]) and g.covers(raw[off:off + n])
    assert g.handed_out(192) and not g.handed_out(191) and not g.handed_out(256)
    g.check()


def test_three_runs_checks_each_fill():
    seen = []

    def run(g):
        seen.append(None if g is None else g.fill)
        return 1 if g is None else g.guarded((3,), torch.float32, "cpu", "x")

    plain, guarded = guarded_alloc.three_runs(run, patched=False)
    assert plain == 1 and seen == [None, 0xFF, 0x00] and [g.fill for g, _ in guarded] == [0xFF, 0x00]
    assert all(g.checked == 1 and not g.live for g, _ in guarded)

    def bad(g):
        if g is not None:
            t = g.guarded((3,), torch.float32, "cpu", "x")
            raw, off, n = _raw(g)
            raw[off + n] = 0x77
    with pytest.raises(AssertionError) as e:
        guarded_alloc.three_runs(bad, patched=False)
    assert re.search(r"rear guard of 'x' \(12 bytes\)", str(e.value))


def test_recorded_sizes():
    lib = types.SimpleNamespace(a_workspace_bytes=lambda n: 10 * n + 3, b_workspace_floats=lambda n, k: n * k, other=lambda: 7)
    orig = (lib.a_workspace_bytes, lib.b_workspace_floats, lib.other)
    with guarded_alloc.recorded_sizes(lib, names=["a_workspace_bytes", "b_workspace_floats"]) as seen:
        assert lib.a_workspace_bytes(2) == 23 and lib.a_workspace_bytes(0) == 3 and lib.b_workspace_floats(3, 5) == 15
        assert lib.b_workspace_floats(0, 5) == 0 and lib.other() == 7
    assert seen == {"a_workspace_bytes": [23, 3], "b_workspace_floats": [60]}             # floats as bytes; a size of 0 is not a buffer
    assert (lib.a_workspace_bytes, lib.b_workspace_floats, lib.other) == orig
    from sylber_amd import _lib
    names = [n for n in _lib.EXPORTS if n.endswith(("_workspace_bytes", "_workspace_floats"))]
    assert "sylber_knn_workspace_bytes" in names and "sylber_condition_units_workspace_floats" in names and len(names) >= 25
