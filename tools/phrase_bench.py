"""Phrase search on one MI355X (csrc/dtw.hip, ``SyllableIndex.search_phrases``), seeded random data on the device, D = 768, L2.

N database rows in sequences of 20 to 60 rows; phrases of m rows, P of them so that the query rows total ``rows``; k = 10.  The
yardstick is ``SyllableIndex.search`` of the same index with the same number of query rows in the same run: the same contraction
without the dynamic programme.  For every (rows, m): median milliseconds of the whole call (host clock around calls that end in a
device synchronise, after a warm-up call), the spread (min .. max) of the timed calls, TFLOP/s on 2 rows N D, and the ratio
yardstick time / phrase-search time.  Prints one JSON line (rows also go to stderr as they finish).

    python tools/phrase_bench.py [--iters 5] [--N 4194304] [--rows 128,1024,8192] [--ms 2,8,32] [--k 10]

``--refined [--storage fp16|bf16] [--refine 4]`` adds the two-stage leg (csrc/dtw16.hip, ``SyllableIndex.search_phrases_refined``): in
the same run, on the same phrases and index, the whole-call time of ``search_phrases_refined(k, refine, storage)`` beside
``search_phrases``'s (``refined_over_phrase`` = two-stage time / ``search_phrases`` time: below 1 is faster), and for refine 1, 2, 4
and 8 the share of phrases whose exact top-k (``recovered_topk``) and whose exact best sequence (``recovered_top1``) the two-stage
call returns.  The 16-bit plane is built before anything is timed.

``--pq [--M 48] [--storage fp16|bf16] [--refine 4]`` (with ``--refined``) adds the compressed leg (csrc/dtwpq.hip,
``PQSyllableIndex.search_phrases``) on codes of the same rows: the whole-call time with the fp32 rows held (``pq_held_ms``: exact
re-rank on the rows) and of the call that runs after ``drop_rows()`` (``pq_dropped_ms``: ``rerank=False``, the exact DTW straight
from the codes; the call is bitwise the same before and after the drop), each over ``search_phrases_refined``'s time in the same
run; for refine 1, 2, 4 and 8 the share of phrases whose exact top-k comes back (rows held: the same list; rows dropped: the same
set of sequences); and the device bytes of each index.  The codebooks are the sub-rows of 256 stored rows drawn at random, not
k-means: the rows are independent gaussian, so training has no structure to find.  Codes, 16-bit codebooks and reconstruction norms
are built before anything is timed.  With ``--align`` also ``pq_align_dropped_ms``: the whole call of
``pq.align_phrases(..., rerank=False)`` on the spans of that ``rerank=False`` search, with the number of pairs aligned
(``pq_align_pairs``).

``--occurrences [--storage fp16|bf16] [--refine 4]`` adds the leg of "every occurrence" (``SyllableIndex.search_occurrences`` and
``search_occurrences_refined``): in the same run, on the same phrases and index, the whole-call time of each beside its
per-sequence sibling's (``occ_over_phrase`` = ``search_occurrences`` / ``search_phrases``, ``occ_refined_over_refined`` =
``search_occurrences_refined`` / ``search_phrases_refined``: above 1 is slower), and the mean number of distinct sequences among a
phrase's k occurrences.  It times ``search_phrases_refined`` itself when ``--refined`` is not given.

``--align [--storage fp16|bf16] [--refine 4]`` adds the leg of the warping paths (csrc/dtw_align.hip, ``SyllableIndex.align_phrases``):
in the same run, on the same phrases and index, the whole-call time of ``align_phrases`` on the spans that the timed
``search_phrases_refined`` call returns, beside that call's time (``align_over_refined`` = ``align_phrases`` / ``search_phrases_refined``),
with the number of pairs aligned, the spans' mean width and the paths' mean number of cells.  It times ``search_phrases_refined``
itself when neither ``--refined`` nor ``--occurrences`` is given.

``--ivf [--nlist 4096] [--centres 20000] [--noise 0.3] [--configs 1:8:4,8:32:4,8:32:12,32:32:4,32:64:8]`` runs the leg of the phrase search
through the inverted file (csrc/phrase_vote.hip, ``IVFSyllableIndex.search_phrases``) INSTEAD of the legs above, on data of its own:
on independent gaussian rows recall of an inverted file means nothing, so the rows are the clustered mixture of tools/ivf_bench.py
(sequences of 20 to 60 rows) and each phrase is m consecutive rows of one sequence plus ``noise`` x gaussian noise.  Per (rows, m),
all from one run: the whole-call time of ``search_phrases`` and ``search_phrases_refined`` (the parent's entry points, the
yardstick), and per ``nprobe:seeds:refine`` the whole-call time of ``ivf.search_phrases``, of ``ivf.search`` alone on the same rows
with ``k = seeds``, of the re-rank alone (``sylber_dtw_rerank`` on the call's candidates, packed before the clock starts), the
remainder (the vote and the host work: packing, tables, the seen count), ``last_search``'s fraction and seen, recall@k against the
exact sequences, the share of phrases whose exact top-k / best sequence comes back and the share whose planted sequence is first.

``--ivfpq [--M 48] [--nlist 4096] [--configs 1:8:4,8:32:4]`` runs the leg of the phrase search on the compressed inverted file
(csrc/dtw_codes.hip, ``IVFPQSyllableIndex.search_phrases``) INSTEAD of the legs above, on the data of ``--ivf``.  The codebooks are the
sub-rows of 256 stored rows (of 256 residuals for ``residual=True``) drawn at random.  Per (rows, m) and ``nprobe:seeds:refine``, all
from one run: the whole-call time of ``ix.search_phrases`` with the rows held (``rerank=True``), after ``drop_rows()`` and with
residual codes after ``drop_rows()``; ``IVFSyllableIndex.search_phrases`` at the same setting and ``PQSyllableIndex.search_phrases``
(rows dropped, ``refine``) beside them; the dropped call's stage 1a (``ix.search`` alone), stage 2 alone and remainder (the vote and
the host work); and stage 2 alone two ways on the same candidates: ``sylber_dtw_rerank_codes``, and ``ix.decode`` of the candidate
sequences' rows into a scratch followed by ``sylber_dtw_rerank`` on it (the candidate copy to the host that sizes the scratch
included), with the scratch's rows.  Lazy state is built before anything is timed.

``--occurrences`` combines with ``--ivf``, ``--ivfpq`` and ``--pq``: each new ``search_occurrences`` is timed beside its per-sequence
sibling in the same process (``ivf_occ_ms`` beside ``ivf_phrase_ms``; ``occ_held_ms`` / ``occ_dropped_ms`` /
``occ_residual_dropped_ms`` / ``pq_occ_dropped_ms`` beside ``held_ms`` / ``dropped_ms`` / ``residual_dropped_ms`` / ``pq_dropped_ms``;
``pq_occ_held_ms`` / ``pq_occ_dropped_ms`` beside ``pq_held_ms`` / ``pq_dropped_ms``).  With ``--ivfpq`` the dropped half then reports the
occurrence calls in place of its stage break-down, and stage 2 alone two ways on the dropped call's candidates:
``sylber_dtw_rerank_occurrences_codes`` on the codes and ``sylber_dtw_rerank_occurrences`` on the decoded plane of the whole index
(``two_entries_same_bits``).  Without ``--ivf`` / ``--ivfpq`` it also times ``sylber_dtw_rerank_occurrences`` alone on
``search_occurrences_refined``'s candidates (``occ_rerank_alone_ms``).

``--repeats R`` (``--ivf`` / ``--ivfpq``) plants each query phrase R times in one sequence -- the phrase is the noisy copy of the
sequence's first m rows, and R - 1 further noisy copies of the phrase are written behind it -- so that occurrences exist;
``*_planted_found`` is the mean number of a phrase's R planted spans that come back among its k (a returned span that shares half of
a planted span's rows counts).  Shapes whose R m exceeds the sequences are left out."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out), min(out), max(out)


def rerank_alone(idx, phrases, lens, cand, k):
    """a closure that runs stage 2 alone (``sylber_dtw_rerank``) on the candidates ``cand [P, m]`` of one call; the packing of the
    phrases, the tables and the buffers are made here, before the clock starts"""
    from sylber_amd import _lib
    from sylber_amd._index import _on_device, _phrase_blocks, _phrase_outputs, _row_norms
    from sylber_amd.kmeans import _stream, _vp
    lib, dev = _lib.load(), idx.device
    lens = np.asarray(lens, np.int64)
    P, m = cand.shape
    off = idx.sequence_offsets()
    off_d = _on_device(off, np.int32, dev)
    b = _phrase_blocks(lib, dev, idx._prep(phrases), lens, 0, P, off, m, 0, 0, None)
    qn = _row_norms(b.qp)
    ws = torch.empty(int(lib.sylber_dtw16_workspace_bytes(P, m, 1)), dtype=torch.uint8, device=dev)
    place_d, len_d = _on_device(b.place, np.int32, dev), _on_device(lens, np.int32, dev)
    c32 = cand.to(torch.int32).contiguous()
    costs, seqs, spans = _phrase_outputs(P, k, dev)

    def run():
        with torch.cuda.device(dev):
            _lib.check(lib.sylber_dtw_rerank(_vp(b.qp), b.nb, _vp(qn), _vp(place_d), _vp(len_d), P, _vp(idx._x), len(idx), idx.dim, _vp(idx._c),
                                             0, _vp(c32), m, _vp(off_d), off.size - 1, k, _vp(costs), _vp(seqs), _vp(spans), _vp(ws),
                                             _stream(dev)), "sylber_dtw_rerank")
    return run


def clustered_index(args, dev, g, rng):
    """the data of the --ivf and --ivfpq legs -> (SyllableIndex, sequence lengths, offsets, the shapes of ``planted_shapes``)"""
    from sylber_amd import SyllableIndex
    D, N = 768, args.N
    lens = rng.integers(20, 61, N // 20 + 1)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), N)) + 1]
    lens[-1] -= int(lens.sum()) - N
    lens = lens[lens > 0]
    off = np.concatenate([[0], np.cumsum(lens)])
    groups = np.repeat(np.arange(lens.size), lens).astype(np.int32)
    cent = 2.0 * torch.randn(args.centres, D, device=dev, generator=g)
    w = torch.rand(args.centres, device=dev, generator=g) ** 3
    x = torch.empty(N, D, device=dev)
    for r0 in range(0, N, 1 << 19):
        n = min(1 << 19, N - r0)
        x[r0:r0 + n] = cent[torch.multinomial(w, n, replacement=True, generator=g)] + torch.randn(n, D, device=dev, generator=g)
    shapes = planted_shapes(args, x, lens, off, dev, g, rng)                # --repeats > 1 writes into x: before the index exists
    return SyllableIndex(x, metric="l2", groups=groups, device=dev), lens, off, shapes


def planted_shapes(args, x, lens, off, dev, g, rng):
    """per (rows, m) of --rows x --ms: ``(m, P, phrases [P m, D], truth [P] on the device, planted [P, R, 2] on the device)``.  A phrase
    is m consecutive rows of its truth sequence plus ``noise`` x gaussian noise (the planted noisy copy).  With ``--repeats R`` > 1 the
    truth sequences are distinct and hold R m rows or more; the phrase comes from the sequence's first m rows and R - 1 further noisy
    copies OF THE PHRASE are written into the next slots of m rows, so that the sequence holds R occurrences: ``planted`` are their spans.
    A shape whose R m exceeds every sequence, or that needs more sequences than there are, is left out."""
    D, R = x.shape[1], args.repeats
    used = np.zeros(lens.size, bool)
    shapes = []
    for rows in [int(v) for v in args.rows.split(",")]:
        for m in [int(v) for v in args.ms.split(",")]:
            P = rows // m
            ok = np.nonzero((lens >= R * m) & ~used)[0]
            if R > 1:
                if ok.size < P:
                    print(json.dumps({"rows": rows, "m": m, "skipped": "fewer than %d free sequences of %d rows" % (P, R * m)}), file=sys.stderr)
                    continue
                truth = rng.choice(ok, P, replace=False)
                used[truth] = True
                start = off[truth]
            else:
                truth = ok[rng.integers(0, ok.size, P)]
                start = off[truth] + (rng.random(P) * (lens[truth] - m + 1)).astype(np.int64)
            pick = torch.from_numpy((start[:, None] + np.arange(m)[None, :]).reshape(-1)).to(dev)
            ph = x[pick] + args.noise * torch.randn(P * m, D, device=dev, generator=g)
            for r in range(1, R):
                x[pick + r * m] = ph + args.noise * torch.randn(P * m, D, device=dev, generator=g)
            first = start[:, None] + m * np.arange(R)[None, :]
            planted = torch.from_numpy(np.stack([first, first + m], 2)).to(dev)
            shapes.append((m, P, ph, torch.from_numpy(truth).to(dev), planted))
    return shapes


def planted_found(spans, planted):
    """the mean number of a phrase's planted spans [P, R, 2] that come back among its k spans [P, k, 2]: a planted span counts when a
    returned one shares at least half of its rows"""
    lo = torch.maximum(spans[:, :, None, 0], planted[:, None, :, 0])
    hi = torch.minimum(spans[:, :, None, 1], planted[:, None, :, 1])
    need = (planted[:, None, :, 1] - planted[:, None, :, 0] + 1) // 2
    return round(float(((hi - lo >= need) & (spans[:, :, None, 0] >= 0)).any(1).sum(1).float().mean()), 3)


def occ_stage2_alone(dev, phrases, lens, cand, k, off, entry, db):
    """a closure that runs stage 2 of an occurrence search alone on the candidates ``cand [P, m]`` of one call: ``entry`` is
    ``sylber_dtw_rerank_occurrences`` with ``db = (rows, N, D, norms)`` or ``sylber_dtw_rerank_occurrences_codes`` with ``db`` = the
    coded-database group, N, D and the norms (L2, the phrases as given).  Packing, tables, buffers and the workspace are made here,
    before the clock starts; one launch, so P m k must stay below 2^30."""
    from sylber_amd import _lib
    from sylber_amd._index import _on_device, _phrase_blocks, _phrase_outputs, _prep, _row_norms
    from sylber_amd.kmeans import _stream, _vp
    lib = _lib.load()
    lens = np.asarray(lens, np.int64)
    P, m = cand.shape
    off_d = _on_device(off, np.int32, dev)
    b = _phrase_blocks(lib, dev, _prep(phrases, "l2", dev), lens, 0, P, off, m, 0, 0, None)
    qn = _row_norms(b.qp)
    ws = torch.empty(int(lib.sylber_dtw_occ_workspace_bytes(P, m, k)), dtype=torch.uint8, device=dev)
    place_d, len_d = _on_device(b.place, np.int32, dev), _on_device(lens, np.int32, dev)
    c32 = cand.to(torch.int32).contiguous()
    costs, seqs, spans = _phrase_outputs(P, k, dev)
    fn = getattr(lib, entry)

    def run():
        with torch.cuda.device(dev):
            _lib.check(fn(_vp(b.qp), b.nb, _vp(qn), _vp(place_d), _vp(len_d), P, *db, 0, _vp(c32), m, _vp(off_d), off.size - 1, k, _vp(costs),
                          _vp(seqs), _vp(spans), _vp(ws), _stream(dev)), entry)
        return costs, seqs, spans
    return run


def codes_rerank_alone(ix, phrases, lens, cand, k):
    """``rerank_alone`` for ``sylber_dtw_rerank_codes`` on ``ix``'s own codes"""
    from sylber_amd import _lib
    from sylber_amd._index import _on_device, _phrase_blocks, _phrase_outputs, _prep, _row_norms
    from sylber_amd.kmeans import _stream, _vp
    lib, dev = _lib.load(), ix.device
    lens = np.asarray(lens, np.int64)
    P, m = cand.shape
    off = ix.sequence_offsets()
    off_d = _on_device(off, np.int32, dev)
    b = _phrase_blocks(lib, dev, _prep(phrases, "l2", dev), lens, 0, P, off, m, 0, 0, None)
    qn = _row_norms(b.qp)
    ws = torch.empty(int(lib.sylber_dtw16_workspace_bytes(P, m, 1)), dtype=torch.uint8, device=dev)
    place_d, len_d = _on_device(b.place, np.int32, dev), _on_device(lens, np.int32, dev)
    c32 = cand.to(torch.int32).contiguous()
    costs, seqs, spans = _phrase_outputs(P, k, dev)
    db, pc = ix._coded_db()

    def run():
        with torch.cuda.device(dev):
            _lib.check(lib.sylber_dtw_rerank_codes(_vp(b.qp), b.nb, _vp(qn), _vp(place_d), _vp(len_d), P, *db, len(ix), ix.dim, _vp(pc), 0,
                                                   _vp(c32), m, _vp(off_d), off.size - 1, k, _vp(costs), _vp(seqs), _vp(spans), _vp(ws),
                                                   _stream(dev)), "sylber_dtw_rerank_codes")
        return costs, seqs, spans
    return run


def decode_rerank_alone(ix, phrases, lens, cand, k):
    """stage 2 the other way: the candidates to the host, ``ix.decode`` of the rows of the distinct candidate sequences into a
    compact scratch, ``sylber_dtw_rerank`` on it, sequence numbers and rows mapped back -> a closure, and a dict that it fills with
    the scratch's rows"""
    from sylber_amd import _lib
    from sylber_amd._index import _on_device, _phrase_blocks, _phrase_outputs, _prep, _row_norms
    from sylber_amd.kmeans import _stream, _vp
    lib, dev = _lib.load(), ix.device
    lens = np.asarray(lens, np.int64)
    P, m = cand.shape
    off = ix.sequence_offsets()
    seq_len = np.diff(off)
    b = _phrase_blocks(lib, dev, _prep(phrases, "l2", dev), lens, 0, P, off, m, 0, 0, None)
    qn = _row_norms(b.qp)
    ws = torch.empty(int(lib.sylber_dtw16_workspace_bytes(P, m, 1)), dtype=torch.uint8, device=dev)
    place_d, len_d = _on_device(b.place, np.int32, dev), _on_device(lens, np.int32, dev)
    costs, seqs, spans = _phrase_outputs(P, k, dev)
    info = {}

    def run():
        cand_h = cand.cpu().numpy()
        uniq = np.unique(cand_h[cand_h >= 0])
        coff = np.concatenate([[0], np.cumsum(seq_len[uniq])]).astype(np.int64)
        rid = np.repeat(off[uniq] - coff[:-1], seq_len[uniq]) + np.arange(coff[-1])
        x = ix.decode(torch.from_numpy(rid).to(dev))
        cn = _row_norms(x)
        uniq_d, coff_d, roff_d = (torch.from_numpy(a).to(dev) for a in (uniq, coff, off[uniq]))
        cc = torch.searchsorted(uniq_d, cand.clamp(min=0))
        cc = torch.where(cand < 0, torch.full_like(cc, -1), cc).to(torch.int32).contiguous()
        with torch.cuda.device(dev):
            _lib.check(lib.sylber_dtw_rerank(_vp(b.qp), b.nb, _vp(qn), _vp(place_d), _vp(len_d), P, _vp(x), int(coff[-1]), ix.dim, _vp(cn), 0,
                                             _vp(cc), m, _vp(coff_d.to(torch.int32)), int(uniq.size), k, _vp(costs), _vp(seqs), _vp(spans),
                                             _vp(ws), _stream(dev)), "sylber_dtw_rerank")
        hit = seqs >= 0
        sc = seqs.clamp(min=0)
        spans.copy_(torch.where(hit[:, :, None], spans - coff_d[sc][:, :, None] + roff_d[sc][:, :, None], spans))
        seqs.copy_(torch.where(hit, uniq_d[sc], seqs))
        info["scratch_rows"] = int(coff[-1])
        return costs, seqs, spans
    return run, info


def sampled_codebooks(rows, M, g):
    """[M, 256, D / M]: the sub-rows of 256 of ``rows`` drawn at random"""
    pick = torch.randperm(rows.shape[0], device=rows.device, generator=g)[:256]
    return rows[pick].reshape(256, M, rows.shape[1] // M).permute(1, 0, 2).contiguous()


def ivfpq_leg(args, dev):
    from sylber_amd import IVFPQSyllableIndex, IVFSyllableIndex, PQSyllableIndex
    from sylber_amd.kmeans import _vp
    g = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    D, N, k, M = 768, args.N, args.k, args.M
    idx, lens, off, shapes = clustered_index(args, dev, g, rng)
    idx.sequence_offsets()
    ivf = IVFSyllableIndex.build(idx, nlist=args.nlist, seed=0, max_iter=args.max_iter, train_rows=args.train_rows)
    cb = sampled_codebooks(idx.features, M, g)
    t0 = time.perf_counter()
    ix = IVFPQSyllableIndex.build(idx, M=M, centroids=ivf.centroids, codebooks=cb)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    lab = ix.labels
    keep = torch.nonzero(lab >= 0).flatten()[:1 << 16]
    rcb = sampled_codebooks(idx.features[keep] - ivf.centroids[lab[keep]], M, g)
    ixr = IVFPQSyllableIndex.build(idx, M=M, centroids=ivf.centroids, codebooks=rcb, residual=True)
    pq = PQSyllableIndex.build(idx, M, codebooks=cb)
    warm = idx.features[:2]
    for i in (ix, ixr):
        i.search_phrases(warm, 1, 1, lengths=[2], rerank=False)              # the lazy state
    pq.search_phrases(warm, 1, 1, args.storage, lengths=[2], rerank=False)
    torch.cuda.synchronize()
    held_bytes = {"ivfpq": ix.nbytes, "ivfpq_residual": ixr.nbytes, "pq": pq.nbytes}
    head = {"D": D, "metric": "l2", "N": N, "sequences": int(lens.size), "nlist": args.nlist, "M": M, "k": k, "iters": args.iters,
            "noise": args.noise, "storage": args.storage, "ivfpq_build_s": round(build_s, 2),
            "data": "synthetic mixture of %d Gaussians, sequences of 20 to 60 rows, planted noisy phrases" % args.centres}
    print(json.dumps(head), file=sys.stderr, flush=True)
    configs = [tuple(int(v) for v in c.split(":")) for c in args.configs.split(",")]
    head["repeats"] = args.repeats
    if args.occurrences:
        for i in (ix, ixr):
            i.search_occurrences(warm, 1, 1, lengths=[2], rerank=False)
        pq.search_occurrences(warm, 1, 1, args.storage, lengths=[2], rerank=False)
        torch.cuda.synchronize()
    out = []
    planted = lambda got, truth_d: round(float((got[1][:, 0] == truth_d).float().mean()), 4)
    for dropped in (False, True):                                             # every rows-held figure first: drop_rows() cannot be undone
        if dropped:
            for i in (ix, ixr, pq):
                i.drop_rows()
        for m, P, ph, truth_d, planted_d in shapes:
            ln = [m] * P
            for nprobe, seeds, refine in configs:
                row = {"rows": P * m, "m": m, "phrases": P, "nprobe": nprobe, "seeds": seeds, "refine": refine}
                kw = dict(seeds=seeds, refine=refine, lengths=ln)
                if not dropped:
                    call = lambda: ix.search_phrases(ph, k, nprobe, seeds=seeds, refine=refine, lengths=ln, rerank=True)
                    t, lo, hi = timed(call, args.iters)
                    t_ivf, _, _ = timed(lambda: ivf.search_phrases(ph, k, nprobe, seeds=seeds, refine=refine, lengths=ln), args.iters)
                    row.update(held_ms=round(t, 2), held_ms_min_max=[round(lo, 2), round(hi, 2)], held_planted_top1=planted(call(), truth_d),
                               ivf_phrase_ms=round(t_ivf, 2))
                    if args.occurrences:
                        occ = lambda: ix.search_occurrences(ph, k, nprobe, rerank=True, **kw)
                        to, lo, hi = timed(occ, args.iters)
                        t_io, lo2, hi2 = timed(lambda: ivf.search_occurrences(ph, k, nprobe, **kw), args.iters)
                        row.update(occ_held_ms=round(to, 2), occ_held_ms_min_max=[round(lo, 2), round(hi, 2)], occ_held_over_held=round(to / t, 3),
                                   occ_held_planted_found=planted_found(occ()[2], planted_d), ivf_occ_ms=round(t_io, 2),
                                   ivf_occ_ms_min_max=[round(lo2, 2), round(hi2, 2)], ivf_occ_over_ivf_phrase=round(t_io / t_ivf, 3),
                                   ivf_occ_planted_found=planted_found(ivf.search_occurrences(ph, k, nprobe, **kw)[2], planted_d))
                elif args.occurrences:                                      # every occurrence from the codes, beside the per-sequence siblings
                    t, lo, hi = timed(lambda: ix.search_phrases(ph, k, nprobe, **kw), args.iters)
                    occ = lambda: ix.search_occurrences(ph, k, nprobe, return_candidates=True, **kw)
                    to, lo_o, hi_o = timed(occ, args.iters)
                    got = occ()
                    t_r, _, _ = timed(lambda: ixr.search_phrases(ph, k, nprobe, **kw), args.iters)
                    occr = lambda: ixr.search_occurrences(ph, k, nprobe, **kw)
                    to_r, lo_r, hi_r = timed(occr, args.iters)
                    t_pq, _, _ = timed(lambda: pq.search_phrases(ph, k, refine, args.storage, lengths=ln), args.iters)
                    occp = lambda: pq.search_occurrences(ph, k, refine, args.storage, lengths=ln)
                    to_pq, lo_p, hi_p = timed(occp, args.iters)
                    db, pc = ix._coded_db()
                    if "plane" not in head:                                  # the decoded plane of the whole index, once: 4 N D bytes
                        head["plane"] = torch.cat([ix.decode(torch.arange(r0, min(N, r0 + (1 << 18)), device=dev)) for r0 in range(0, N, 1 << 18)])
                    codes_run = occ_stage2_alone(dev, ph, ln, got[3], k, off, "sylber_dtw_rerank_occurrences_codes", db + (N, D, _vp(pc)))
                    plane_run = occ_stage2_alone(dev, ph, ln, got[3], k, off, "sylber_dtw_rerank_occurrences", (_vp(head["plane"]), N, D, _vp(pc)))
                    t_codes, lo_c, hi_c = timed(codes_run, args.iters)
                    t_plane, lo_f, hi_f = timed(plane_run, args.iters)
                    a, b = codes_run(), plane_run()
                    same = all(torch.equal(u, v) for u, v in zip(a, b)) and all(torch.equal(u, v) for u, v in zip(a, got[:3]))
                    sq = got[1].sort(1).values
                    row.update(dropped_ms=round(t, 2), dropped_ms_min_max=[round(lo, 2), round(hi, 2)], occ_dropped_ms=round(to, 2),
                               occ_dropped_ms_min_max=[round(lo_o, 2), round(hi_o, 2)], occ_dropped_over_dropped=round(to / t, 3),
                               occ_dropped_planted_found=planted_found(got[2], planted_d), residual_dropped_ms=round(t_r, 2),
                               occ_residual_dropped_ms=round(to_r, 2), occ_residual_dropped_ms_min_max=[round(lo_r, 2), round(hi_r, 2)],
                               occ_residual_over_residual=round(to_r / t_r, 3), occ_residual_planted_found=planted_found(occr()[2], planted_d),
                               pq_dropped_ms=round(t_pq, 2), pq_occ_dropped_ms=round(to_pq, 2), pq_occ_dropped_ms_min_max=[round(lo_p, 2), round(hi_p, 2)],
                               pq_occ_over_pq=round(to_pq / t_pq, 3), pq_occ_planted_found=planted_found(occp()[2], planted_d),
                               occ_codes_entry_ms=round(t_codes, 2), occ_codes_entry_ms_min_max=[round(lo_c, 2), round(hi_c, 2)],
                               occ_fp32_entry_on_decoded_plane_ms=round(t_plane, 2), occ_fp32_entry_ms_min_max=[round(lo_f, 2), round(hi_f, 2)],
                               occ_codes_over_fp32=round(t_codes / t_plane, 3), two_entries_same_bits=same,
                               occ_distinct_sequences=round(float((1 + (sq[:, 1:] != sq[:, :-1]).sum(1)).float().mean()), 2))
                else:
                    call = lambda: ix.search_phrases(ph, k, nprobe, seeds=seeds, refine=refine, lengths=ln, return_candidates=True)
                    t, lo, hi = timed(call, args.iters)
                    got = call()
                    ls = ix.last_search
                    callr = lambda: ixr.search_phrases(ph, k, nprobe, seeds=seeds, refine=refine, lengths=ln)
                    t_r, lo_r, hi_r = timed(callr, args.iters)
                    t_pq, _, _ = timed(lambda: pq.search_phrases(ph, k, refine, args.storage, lengths=ln), args.iters)
                    t_seed, _, _ = timed(lambda: ix.search(ph, seeds, nprobe), args.iters)
                    codes_run = codes_rerank_alone(ix, ph, ln, got[3], k)
                    decode_run, info = decode_rerank_alone(ix, ph, ln, got[3], k)
                    t_codes, _, _ = timed(codes_run, args.iters)
                    t_dec, _, _ = timed(decode_run, args.iters)
                    a, b = codes_run(), decode_run()
                    same = all(torch.equal(u, v) for u, v in zip(a, b)) and all(torch.equal(u, v) for u, v in zip(a, got[:3]))
                    cols = int((torch.from_numpy(np.diff(off)).to(dev)[got[3].clamp(min=0)] * (got[3] >= 0)).sum())
                    row.update(dropped_ms=round(t, 2), dropped_ms_min_max=[round(lo, 2), round(hi, 2)], dropped_planted_top1=planted(got, truth_d),
                               residual_dropped_ms=round(t_r, 2), residual_dropped_ms_min_max=[round(lo_r, 2), round(hi_r, 2)],
                               residual_planted_top1=planted(callr(), truth_d), pq_dropped_ms=round(t_pq, 2), seed_search_ms=round(t_seed, 2),
                               rerank_codes_ms=round(t_codes, 2), remainder_ms=round(t - t_seed - t_codes, 2), decode_then_rerank_ms=round(t_dec, 2),
                               codes_over_decode=round(t_codes / t_dec, 3), two_ways_same_bits=same, scratch_rows=info["scratch_rows"],
                               pair_columns=cols, fraction=round(ls["fraction"], 6), seen=round(ls["seen"], 1))
                print(json.dumps(row), file=sys.stderr, flush=True)
                out.append(row)
    head.pop("plane", None)
    head.update(rows=out, device_bytes={"syllable_index_rows_norms_groups": 4 * N * D + 8 * N, "rows_held": held_bytes,
                                        "rows_dropped": {"ivfpq": ix.nbytes, "ivfpq_residual": ixr.nbytes, "pq": pq.nbytes}})
    print(json.dumps(head))


def ivf_leg(args, dev):
    from sylber_amd import IVFSyllableIndex
    g = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    D, N, k = 768, args.N, args.k
    idx, lens, off, shapes = clustered_index(args, dev, g, rng)
    idx.sequence_offsets()
    idx.half_rows(args.storage)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ivf = IVFSyllableIndex.build(idx, nlist=args.nlist, seed=0, max_iter=args.max_iter, train_rows=args.train_rows)
    torch.cuda.synchronize()
    head = {"D": D, "metric": "l2", "N": N, "sequences": int(lens.size), "nlist": args.nlist, "k": k, "iters": args.iters, "noise": args.noise,
            "storage": args.storage, "build_s": round(time.perf_counter() - t0, 2),
            "data": "synthetic mixture of %d Gaussians, sequences of 20 to 60 rows, planted noisy phrases" % args.centres}
    print(json.dumps(head), file=sys.stderr, flush=True)
    configs = [tuple(int(v) for v in c.split(":")) for c in args.configs.split(",")]
    out = []
    head["repeats"] = args.repeats
    for m, P, ph, truth_d, planted_d in shapes:
        ln = [m] * P
        t_exact, lo, hi = timed(lambda: idx.search_phrases(ph, k, lengths=ln), min(args.iters, 2))
        exact = idx.search_phrases(ph, k, lengths=ln)[1]
        t_ref, lo2, hi2 = timed(lambda: idx.search_phrases_refined(ph, k, args.refine, args.storage, lengths=ln), args.iters)
        base = {"rows": P * m, "m": m, "phrases": P, "phrase_ms": round(t_exact, 2), "phrase_ms_min_max": [round(lo, 2), round(hi, 2)],
                "refined_ms": round(t_ref, 2), "refined_ms_min_max": [round(lo2, 2), round(hi2, 2)], "refined_refine": args.refine,
                "exact_planted_top1": round(float((exact[:, 0] == truth_d).float().mean()), 4)}
        for nprobe, seeds, refine in configs:
            if nprobe > min(args.nlist, 128) or k * refine > 128:
                continue
            call = lambda: ivf.search_phrases(ph, k, nprobe, seeds=seeds, refine=refine, lengths=ln, return_candidates=True)
            t, lo, hi = timed(call, args.iters)
            got = call()
            ls = dict(ivf.last_search)
            t_seed, _, _ = timed(lambda: ivf.search(ph, seeds, nprobe), args.iters)
            t_rr, _, _ = timed(rerank_alone(idx, ph, ln, got[3], k), args.iters)
            row = dict(base, nprobe=nprobe, seeds=seeds, refine=refine, ivf_phrase_ms=round(t, 2), ivf_phrase_ms_min_max=[round(lo, 2), round(hi, 2)],
                       seed_search_ms=round(t_seed, 2), rerank_ms=round(t_rr, 2), remainder_ms=round(t - t_seed - t_rr, 2),
                       over_refined=round(t / t_ref, 3), over_phrase=round(t / t_exact, 3), fraction=round(ls["fraction"], 6),
                       seen=round(ls["seen"], 1),
                       recall_at_k=round(float(((got[1][:, :, None] == exact[:, None, :]) & (exact[:, None, :] >= 0)).any(1).sum())
                                         / max(1, int((exact >= 0).sum())), 4), recovered_topk=round(float((got[1] == exact).all(1).float().mean()), 4),
                       recovered_top1=round(float((got[1][:, 0] == exact[:, 0]).float().mean()), 4),
                       planted_top1=round(float((got[1][:, 0] == truth_d).float().mean()), 4))
            if args.occurrences:
                occ = lambda: ivf.search_occurrences(ph, k, nprobe, seeds=seeds, refine=refine, lengths=ln)
                to, lo, hi = timed(occ, args.iters)
                row.update(ivf_occ_ms=round(to, 2), ivf_occ_ms_min_max=[round(lo, 2), round(hi, 2)], ivf_occ_over_ivf_phrase=round(to / t, 3),
                           ivf_occ_planted_found=planted_found(occ()[2], planted_d))
            print(json.dumps(row), file=sys.stderr, flush=True)
            out.append(row)
    head["rows"] = out
    print(json.dumps(head))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--N", type=int, default=4194304)
    ap.add_argument("--rows", default="128,1024,8192")
    ap.add_argument("--ms", default="2,8,32")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--refined", action="store_true")
    ap.add_argument("--storage", default="fp16", choices=["fp16", "bf16"])
    ap.add_argument("--refine", type=int, default=4)
    ap.add_argument("--occurrences", action="store_true")
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--align", action="store_true")
    ap.add_argument("--pq", action="store_true")
    ap.add_argument("--M", type=int, default=48)
    ap.add_argument("--ivf", action="store_true")
    ap.add_argument("--ivfpq", action="store_true")
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--centres", type=int, default=20000)
    ap.add_argument("--noise", type=float, default=0.3)
    ap.add_argument("--configs", default="1:8:4,8:32:4,8:32:12,32:32:4,32:64:8")
    ap.add_argument("--max-iter", type=int, default=10)
    ap.add_argument("--train-rows", type=int, default=524288)
    args = ap.parse_args()
    from sylber_amd import SyllableIndex
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    if args.ivf:
        return ivf_leg(args, dev)
    if args.ivfpq:
        return ivfpq_leg(args, dev)
    g = torch.Generator(device=dev).manual_seed(0)
    rng = np.random.default_rng(0)
    D, N, k = 768, args.N, args.k
    lens = rng.integers(20, 61, N // 20 + 1)
    lens = lens[:int(np.searchsorted(np.cumsum(lens), N)) + 1]
    lens[-1] -= int(lens.sum()) - N
    lens = lens[lens > 0]
    groups = np.repeat(np.arange(lens.size), lens).astype(np.int32)
    idx = SyllableIndex(torch.randn(N, D, device=dev, generator=g), metric="l2", groups=groups, device=dev)
    idx.sequence_offsets()
    if args.refined or args.occurrences or args.align:
        idx.half_rows(args.storage)
    pq = None
    if args.pq:
        if not args.refined:
            ap.error("--pq is measured beside search_phrases_refined: pass --refined too")
        from sylber_amd import PQSyllableIndex
        pick = torch.randperm(N, device=dev, generator=g)[:256]
        cb = idx.features[pick].reshape(256, args.M, D // args.M).permute(1, 0, 2).contiguous()
        pq = PQSyllableIndex.build(idx, args.M, codebooks=cb)
        pq.search_phrases(idx.features[:2], 1, 1, args.storage, lengths=[2])
    out = []
    for rows in [int(v) for v in args.rows.split(",")]:
        q = idx.features[torch.randint(0, N - rows, (1,), device=dev, generator=g).item():][:rows] + 0.5 * torch.randn(rows, D, device=dev, generator=g)
        fl = 2.0 * rows * N * D
        t_knn, lo, hi = timed(lambda: idx.search(q, k), args.iters)
        base = {"rows": rows, "N": N, "sequences": int(lens.size), "k": k, "search_ms": round(t_knn, 2), "search_ms_min_max": [round(lo, 2), round(hi, 2)],
                "search_tflops": round(fl / t_knn / 1e9, 1)}
        for m in [int(v) for v in args.ms.split(",")]:
            P = rows // m
            t, lo, hi = timed(lambda: idx.search_phrases(q[:P * m], k, lengths=[m] * P), args.iters)
            row = dict(base, m=m, phrases=P, phrase_ms=round(t, 2), phrase_ms_min_max=[round(lo, 2), round(hi, 2)],
                       phrase_tflops=round(2.0 * P * m * N * D / t / 1e9, 1), search_over_phrase=round(t_knn / t, 3))
            if args.refined:
                ph, ln = q[:P * m], [m] * P
                t2, lo, hi = timed(lambda: idx.search_phrases_refined(ph, k, args.refine, args.storage, lengths=ln), args.iters)
                exact = idx.search_phrases(ph, k, lengths=ln)[1]
                share = {}
                for r in (1, 2, 4, 8):
                    if k * r > 128:
                        continue
                    got = idx.search_phrases_refined(ph, k, r, args.storage, lengths=ln)[1]
                    share[str(r)] = [round(float((got == exact).all(1).float().mean()), 4), round(float((got[:, 0] == exact[:, 0]).float().mean()), 4)]
                row.update(storage=args.storage, refine=args.refine, refined_ms=round(t2, 2), refined_ms_min_max=[round(lo, 2), round(hi, 2)],
                           refined_over_phrase=round(t2 / t, 3), recovered_topk={r: v[0] for r, v in share.items()},
                           recovered_top1={r: v[1] for r, v in share.items()})
            if args.occurrences:
                ph, ln = q[:P * m], [m] * P
                if not args.refined:
                    t2, lo, hi = timed(lambda: idx.search_phrases_refined(ph, k, args.refine, args.storage, lengths=ln), args.iters)
                    row.update(storage=args.storage, refine=args.refine, refined_ms=round(t2, 2), refined_ms_min_max=[round(lo, 2), round(hi, 2)])
                t5, lo5, hi5 = timed(lambda: idx.search_occurrences(ph, k, lengths=ln), args.iters)
                t6, lo6, hi6 = timed(lambda: idx.search_occurrences_refined(ph, k, args.refine, args.storage, lengths=ln), args.iters)
                cand = idx.search_occurrences_refined(ph, k, args.refine, args.storage, lengths=ln, return_candidates=True)[3]
                from sylber_amd.kmeans import _vp
                t8, lo8, hi8 = timed(occ_stage2_alone(dev, ph, ln, cand, k, idx.sequence_offsets(), "sylber_dtw_rerank_occurrences",
                                                      (_vp(idx._x), N, D, _vp(idx._c))), args.iters)
                row.update(occ_rerank_alone_ms=round(t8, 3), occ_rerank_alone_ms_min_max=[round(lo8, 3), round(hi8, 3)])
                sq = idx.search_occurrences(ph, k, lengths=ln)[1].sort(1).values
                distinct = 1 + (sq[:, 1:] != sq[:, :-1]).sum(1)
                row.update(occ_ms=round(t5, 2), occ_ms_min_max=[round(lo5, 2), round(hi5, 2)], occ_over_phrase=round(t5 / t, 3),
                           occ_refined_ms=round(t6, 2), occ_refined_ms_min_max=[round(lo6, 2), round(hi6, 2)],
                           occ_refined_over_refined=round(t6 / t2, 3), occ_distinct_sequences=round(float(distinct.float().mean()), 2))
            if args.align:
                ph, ln = q[:P * m], [m] * P
                if not (args.refined or args.occurrences):
                    t2, lo, hi = timed(lambda: idx.search_phrases_refined(ph, k, args.refine, args.storage, lengths=ln), args.iters)
                    row.update(storage=args.storage, refine=args.refine, refined_ms=round(t2, 2), refined_ms_min_max=[round(lo, 2), round(hi, 2)])
                spans = idx.search_phrases_refined(ph, k, args.refine, args.storage, lengths=ln)[2]
                t7, lo7, hi7 = timed(lambda: idx.align_phrases(ph, spans, lengths=ln), args.iters)
                steps = idx.align_phrases(ph, spans, lengths=ln)[1]
                hit = spans[:, :, 0] >= 0
                row.update(align_ms=round(t7, 2), align_ms_min_max=[round(lo7, 2), round(hi7, 2)], align_over_refined=round(t7 / t2, 3),
                           align_pairs=int(hit.sum()), span_mean_width=round(float((spans[:, :, 1] - spans[:, :, 0])[hit].float().mean()), 2),
                           path_mean_steps=round(float(steps[hit].float().mean()), 2))
            if pq is not None:
                t3, lo3, hi3 = timed(lambda: pq.search_phrases(ph, k, args.refine, args.storage, lengths=ln, rerank=True), args.iters)
                t4, lo4, hi4 = timed(lambda: pq.search_phrases(ph, k, args.refine, args.storage, lengths=ln, rerank=False), args.iters)
                want = exact.sort(1).values
                held, dropped = {}, {}
                for r in (1, 2, 4, 8):
                    if k * r > 128:
                        continue
                    got = pq.search_phrases(ph, k, r, args.storage, lengths=ln, rerank=True)[1]
                    held[str(r)] = round(float((got == exact).all(1).float().mean()), 4)
                    got = pq.search_phrases(ph, k, r, args.storage, lengths=ln, rerank=False)[1]
                    dropped[str(r)] = round(float((got.sort(1).values == want).all(1).float().mean()), 4)
                if args.occurrences:
                    t9, lo9, hi9 = timed(lambda: pq.search_occurrences(ph, k, args.refine, args.storage, lengths=ln, rerank=True), args.iters)
                    t10, lo10, hi10 = timed(lambda: pq.search_occurrences(ph, k, args.refine, args.storage, lengths=ln, rerank=False), args.iters)
                    row.update(pq_occ_held_ms=round(t9, 2), pq_occ_held_ms_min_max=[round(lo9, 2), round(hi9, 2)], pq_occ_held_over_pq_held=round(t9 / t3, 3),
                               pq_occ_dropped_ms=round(t10, 2), pq_occ_dropped_ms_min_max=[round(lo10, 2), round(hi10, 2)],
                               pq_occ_dropped_over_pq_dropped=round(t10 / t4, 3))
                if args.align:
                    pspans = pq.search_phrases(ph, k, args.refine, args.storage, lengths=ln, rerank=False)[2]
                    t11, lo11, hi11 = timed(lambda: pq.align_phrases(ph, pspans, lengths=ln, rerank=False), args.iters)
                    row.update(pq_align_dropped_ms=round(t11, 2), pq_align_dropped_ms_min_max=[round(lo11, 2), round(hi11, 2)],
                               pq_align_pairs=int((pspans[:, :, 0] >= 0).sum()))
                row.update(M=args.M, pq_held_ms=round(t3, 2), pq_held_ms_min_max=[round(lo3, 2), round(hi3, 2)], pq_dropped_ms=round(t4, 2),
                           pq_dropped_ms_min_max=[round(lo4, 2), round(hi4, 2)], pq_held_over_refined=round(t3 / t2, 3),
                           pq_dropped_over_refined=round(t4 / t2, 3), pq_recovered_topk_held=held, pq_recovered_topk_dropped=dropped)
            print(json.dumps(row), file=sys.stderr, flush=True)
            out.append(row)
    res = {"D": D, "metric": "l2", "iters": args.iters, "rows": out}
    if pq is not None:
        held = pq.nbytes
        pq.drop_rows()
        res["device_bytes"] = {"syllable_index_rows_norms_groups_plane": 4 * N * D + 4 * N + 4 * N + 2 * N * D, "pq_rows_held": held,
                               "pq_rows_dropped": pq.nbytes}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
