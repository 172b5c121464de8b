"""PinnedOutputPool (sylber_amd/segmenter.py): the leased host blocks behind the numpy results of Segmenter.__call__
(the reference's `.cpu().numpy()` hand-over, sylber/model/sylber.py:122-138).  Host logic only: pageable memory is injected
in place of page-locked memory, so this runs without a GPU; the Segmenter-level behaviour is in tests/test_gpu_e2e.py."""
import gc
import threading

import numpy as np
import torch

from sylber_amd.segmenter import PinnedOutputPool


def _pool(n=2):
    return PinnedOutputPool(max_leased=n, alloc=lambda cap: torch.empty(cap, dtype=torch.uint8))


def test_blocks_are_reused_and_allocations_stop_growing():
    pool = _pool(2)
    for i in range(10):
        owner, blk = pool.lease(3 << 20)
        owner[:4] = i
        assert owner.nbytes >= 3 << 20 and owner.nbytes % PinnedOutputPool.GRANULE == 0
        del owner, blk
        gc.collect()
    assert pool.allocations == 1 and pool.leased == 0


def test_results_stay_intact_while_a_view_is_alive():
    pool = _pool(2)
    owner, _ = pool.lease(1 << 20)
    view = owner[16:32].view(np.float32)          # what a caller keeps: a numpy view whose .base chain ends at the owner
    view[:] = 7.0
    del owner, _
    gc.collect()
    assert pool.leased == 1                       # the view keeps the block out
    other, _b = pool.lease(1 << 20)               # a later call gets ANOTHER block
    other[:] = 0
    assert np.all(view == 7.0) and pool.allocations == 2
    del view
    gc.collect()
    assert pool.leased == 1
    del other, _b
    gc.collect()
    assert pool.leased == 0


def test_fallback_beyond_max_leased_and_recovery():
    pool = _pool(2)
    a = pool.lease(100)
    b = pool.lease(100)
    assert pool.lease(100) is None                # the caller falls back to pageable copies
    del a
    gc.collect()
    c = pool.lease(100)
    assert c is not None and pool.allocations == 2
    del b, c
    gc.collect()
    assert pool.leased == 0


def test_too_small_block_is_dropped_not_hoarded():
    pool = _pool(1)
    a = pool.lease(1 << 20)
    del a
    gc.collect()
    b = pool.lease(4 << 20)                       # the free 1-MiB block cannot serve this: replaced, not kept beside it
    assert b is not None and b[0].nbytes >= 4 << 20 and pool.allocations == 2
    del b
    gc.collect()
    assert pool.leased == 0 and len(pool._free) == 1


def test_release_from_a_finalizer_inside_lease_does_not_deadlock():
    """owner arrays caught in a reference cycle are freed by a collection that can start at any allocation, e.g. inside
    lease() while it holds the pool's lock: the release path must not take that lock"""
    pool = _pool(4)

    class Box:
        pass
    box = Box()
    box.owner, box.blk = pool.lease(100)
    box.me = box                                   # cycle: only the cycle collector frees it
    del box
    real_alloc = pool._alloc

    def alloc_with_gc(cap):
        gc.collect()                               # the collection runs the finalizer on THIS thread (no lock held: allocation is outside it)
        return real_alloc(cap)
    pool._alloc = alloc_with_gc
    done = []

    def run():
        with pool._lock:                           # worst case: a finalizer firing while the lock is held
            gc.collect()
        done.append(pool.lease(200))
    t = threading.Thread(target=run)
    t.start()
    t.join(20)
    assert not t.is_alive(), "deadlock: _release waited for the pool lock"
    assert done and done[0] is not None and pool.leased == 1


def test_trim_after_a_temporarily_raised_budget():
    """Segmenter.stream raises max_leased by its batches in flight and restores it: the extra free blocks must not stay hoarded"""
    pool = _pool(2)
    pool.max_leased = 5
    leases = [pool.lease(1 << 20) for _ in range(5)]
    assert all(l is not None for l in leases) and pool.allocations == 5
    del leases
    gc.collect()
    assert pool.leased == 0 and len(pool._free) == 5
    pool.max_leased = 2
    pool.trim()
    assert len(pool._free) == 2
    a = pool.lease(1 << 20); b = pool.lease(1 << 20)
    assert a is not None and b is not None and pool.lease(1 << 20) is None and pool.allocations == 5


def test_segment_slot_sizing_decays_with_the_recent_batches():
    """Segmenter._note_segments: the block size follows the recent per-batch maximum (`_kcap_seen` only grew)"""
    import collections
    from sylber_amd.segmenter import Segmenter
    s = Segmenter.__new__(Segmenter)
    s._kcap_seen, s._kcap_recent = 128, collections.deque(maxlen=16)
    s._note_segments(40)
    assert s._kcap_seen == 128                     # floor
    s._note_segments(700)                          # one long-clip batch
    assert s._kcap_seen == 704
    for _ in range(16):
        s._note_segments(45)
    assert s._kcap_seen == 128                     # ... forgotten 16 batches later


def test_block_layout_offsets_and_views():
    """Segmenter's host block of one batch: [hidden states | tables | pooled features | counts], each part 256-byte aligned"""
    from sylber_amd.segmenter import _BlockLayout
    lay = _BlockLayout(3, 5, 4, 2, True, True)
    assert (lay.o_seg, lay.o_feat, lay.o_cnt, lay.nbytes) == (256, 512, 768, 1024)
    lean = _BlockLayout(3, 5, 4, 2, False, False)
    assert (lean.o_seg, lean.o_feat, lean.o_cnt, lean.nbytes) == (0, 256, 256, 512)
    assert lean.hidden(np.zeros(512, np.uint8)) is None and lean.tables(np.zeros(512, np.uint8))[1] is None
    blk = torch.zeros(lay.nbytes, dtype=torch.uint8)
    owner = blk.numpy()
    h, c, (s, f) = lay.hidden(blk), lay.counts(blk), lay.tables(blk)
    assert (h.dtype, h.shape, c.dtype, c.shape, s.dtype, s.shape, f.dtype, f.shape) == (
        torch.float32, (3, 5, 4), torch.int32, (3,), torch.int64, (3, 2, 2), torch.float32, (3, 2, 4))
    h.fill_(1.5); c.copy_(torch.tensor([2, 0, 1], dtype=torch.int32)); s.fill_(7); f.fill_(-2.0)
    hn, cn, (sn, fn) = lay.hidden(owner), lay.counts(owner), lay.tables(owner)
    assert np.all(hn == 1.5) and cn.tolist() == [2, 0, 1] and np.all(sn == 7) and np.all(fn == -2.0)   # the parts do not overlap
    s1, f1 = lay.tables(owner, 1)                 # fewer slots: packed at the start of each part
    assert s1.shape == (3, 1, 2) and f1.shape == (3, 1, 4) and np.shares_memory(s1, sn) and np.shares_memory(f1, fn)


def test_result_dicts_on_a_synthetic_block():
    """the per-utterance dicts of __call__, stream and ShardedSegmenter from one leased block: an utterance without segments, in_second,
    frames cuts, and views of a block handed to the caller against copies out of a block that is reused"""
    from sylber_amd.segmenter import _BlockLayout, _result_dicts
    rng = np.random.default_rng(0)
    lay = _BlockLayout(3, 6, 4, 3, True, True)
    owner, _ = _pool(1).lease(lay.nbytes)
    hidden, nseg, (seg, feats) = lay.hidden(owner), lay.counts(owner), lay.tables(owner)
    hidden[:] = rng.standard_normal(hidden.shape)
    nseg[:] = [2, 0, 3]
    seg[:] = rng.integers(0, 6, size=seg.shape)
    feats[:] = rng.standard_normal(feats.shape)
    frames = [6, 4, 1]
    for handed in (True, False):
        out = _result_dicts(nseg, seg, feats, hidden, frames=frames, in_second=False, handed=handed)
        assert [list(o) for o in out] == [["segments", "segment_features", "hidden_states"]] * 3
        for i, o in enumerate(out):
            n = int(nseg[i])
            assert o["hidden_states"].shape == (frames[i], 4) and np.array_equal(o["hidden_states"], hidden[i, :frames[i]])
            assert np.shares_memory(o["hidden_states"], owner) == handed
            if n:
                assert o["segments"].dtype == np.int64 and np.array_equal(o["segments"], seg[i, :n]) and not np.shares_memory(o["segments"], owner)
                assert np.array_equal(o["segment_features"], feats[i, :n]) and np.shares_memory(o["segment_features"], owner) == handed
            else:
                assert o["segments"].shape == (0,) and o["segment_features"].shape == (0,)
    sec = _result_dicts(nseg, seg, None, None, in_second=True)
    assert [list(o) for o in sec] == [["segments"]] * 3
    assert sec[0]["segments"].dtype == np.float64 and np.array_equal(sec[0]["segments"], seg[0, :2] / 50.0) and sec[1]["segments"].shape == (0,)
    full = _result_dicts(nseg, seg, feats, hidden, handed=True)
    assert all(o["hidden_states"].shape == (6, 4) for o in full)     # no frames: the padded length, as the reference


def test_fetch_tables_of_an_overflowing_batch():
    """a batch with more segments than its block has slots: the first k slots of the tables (and pooled features) in a block of their own"""
    from sylber_amd.segmenter import _fetch_tables
    seg = torch.arange(3 * 6 * 2, dtype=torch.int64).view(3, 6, 2)
    feats = torch.randn(3, 6, 4)
    blocks = []

    def alloc(n):
        blocks.append(torch.zeros(n, dtype=torch.uint8))
        return blocks[-1]
    seg_h, feats_h = _fetch_tables(seg, feats, 4, alloc=alloc)
    assert len(blocks) == 1 and np.shares_memory(seg_h, blocks[0].numpy())
    assert np.array_equal(seg_h, seg[:, :4].numpy()) and np.array_equal(feats_h, feats[:, :4].numpy())
    seg_h, feats_h = _fetch_tables(seg, None, 5, alloc=alloc)
    assert feats_h is None and np.array_equal(seg_h, seg[:, :5].numpy())
