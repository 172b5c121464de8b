"""CPU tier: the C-ABI library builds for gfx950, loads, and exports every symbol that
include/sylber_hip.h declares (no compute calls without a GPU)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from sylber_amd import build, _lib
    build.build()
    return _lib.load()


def test_header_symbols_are_exported(lib):
    hdr = open(os.path.join(ROOT, "include", "sylber_hip.h")).read()
    declared = set(re.findall(r"\b(sylber_[a-z0-9_]+)\s*\(", hdr))
    declared.discard("sylber_ctx")
    assert {"sylber_create", "sylber_forward", "sylber_segment", "sylber_destroy", "sylber_last_error"} <= declared
    for name in sorted(declared):
        assert hasattr(lib, name), name
    from sylber_amd import _lib
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)
    # development aids live in their own header and are not part of the drop-in ABI
    dev = open(os.path.join(ROOT, "include", "sylber_hip_dev.h")).read()
    dev_declared = set(re.findall(r"\b(sylber_[a-z0-9_]+)\s*\(", dev))
    assert dev_declared == set(_lib.DEV_EXPORTS) and not (dev_declared & declared)
    for name in sorted(dev_declared):
        assert hasattr(lib, name), name


def test_front_half_taps_are_declared_on_both_sides(lib):
    """the negative stop stages (taps inside the front half) carry the same ids in the header and in the ctypes binding, and the debug
    getter of conv0's GroupNorm table is a development aid, not part of the drop-in ABI"""
    from sylber_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "sylber_hip.h")).read()
    ids = {k: int(v) for k, v in re.findall(r"\b(SYLBER_TAP_[A-Z0-9]+)\s*=\s*(-?\d+)", hdr)}
    assert ids == {"SYLBER_TAP_CONV0": _lib.TAP_CONV0, "SYLBER_TAP_PROJ": _lib.TAP_PROJ, "SYLBER_TAP_POSCONV": _lib.TAP_POSCONV}
    assert sorted(ids.values()) == [-3, -2, -1]
    # the taps inside an encoder layer: SYLBER_TAP_LAYER(l, k) = -(8 (l + 1) + k) with the k names of SYLBER_LTAP_*
    ltap = {k: int(v) for k, v in re.findall(r"\b(SYLBER_LTAP_[A-Z0-9_]+)\s*=\s*(\d+)", hdr)}
    assert ltap == {"SYLBER_LTAP_QKV": _lib.LTAP_QKV, "SYLBER_LTAP_CTX": _lib.LTAP_CTX, "SYLBER_LTAP_ATTN_SUM": _lib.LTAP_ATTN_SUM,
                    "SYLBER_LTAP_LN1": _lib.LTAP_LN1, "SYLBER_LTAP_FFN1": _lib.LTAP_FFN1, "SYLBER_LTAP_FFN2_SUM": _lib.LTAP_FFN2_SUM}
    assert sorted(ltap.values()) == list(range(6)) and sorted(_lib.LTAP_WIDTH) == list(range(6))
    assert re.search(r"#define\s+SYLBER_TAP_LAYER\(l,\s*k\)\s+\(-\(8\s*\*\s*\(\(l\)\s*\+\s*1\)\s*\+\s*\(k\)\)\)", hdr)
    assert _lib.TAP_LAYER(0, 0) == -8 and _lib.TAP_LAYER(1, 5) == -21
    assert "sylber_debug_conv0_scale_shift" in _lib.DEV_EXPORTS and "sylber_debug_conv0_scale_shift" not in _lib.EXPORTS
    dev = open(os.path.join(ROOT, "include", "sylber_hip_dev.h")).read()
    assert re.search(r"int\s+sylber_debug_conv0_scale_shift\s*\(\s*sylber_t\s+h\s*,\s*int32_t\s+B\s*,\s*float\s*\*\s*out_host\s*\)", dev)
    # host-only behaviour: a null handle is refused by both entry points (no device is touched)
    assert lib.sylber_set_stop_stage(None, -1) != 0 and lib.sylber_debug_conv0_scale_shift(None, 1, None) != 0


def test_decoder_taps_are_declared_on_both_sides(lib):
    """the resynthesis decoder's tap stages (include/sylber_hip_dev.h SYLBER_CFM_TAP_* / SYLBER_CFM_BTAP_* / SYLBER_CFM_TAP) carry the same ids
    in the header and in the ctypes binding; the entry points are development aids, and refuse a null handle without touching a device"""
    from sylber_amd import _lib
    dev = open(os.path.join(ROOT, "include", "sylber_hip_dev.h")).read()
    front = {k: int(v) for k, v in re.findall(r"\b(SYLBER_CFM_TAP_[A-Z0-9]+)\s*=\s*(\d+)", dev)}
    assert front == {"SYLBER_CFM_TAP_CONDX": _lib.CFM_TAP_CONDX, "SYLBER_CFM_TAP_GB": _lib.CFM_TAP_GB, "SYLBER_CFM_TAP_XE": _lib.CFM_TAP_XE,
                     "SYLBER_CFM_TAP_X0": _lib.CFM_TAP_X0}
    btap = {k: int(v) for k, v in re.findall(r"\b(SYLBER_CFM_BTAP_[A-Z0-9_]+)\s*=\s*(\d+)", dev)}
    assert btap == {"SYLBER_CFM_BTAP_" + n: getattr(_lib, "CFM_BTAP_" + n)
                    for n in ("H_ATTN", "QKV", "Q", "K", "VT", "QKVF", "CTX", "X_ATTN", "H_FF", "FF", "G", "X_FF")}
    assert sorted(btap.values()) == list(range(12)) and sorted(front.values()) == [1, 2, 3, 4]
    assert re.search(r"#define\s+SYLBER_CFM_TAP\(block,\s*k\)\s+\(16\s*\*\s*\(\(block\)\s*\+\s*1\)\s*\+\s*\(k\)\)", dev)
    assert _lib.CFM_TAP(0, 0) == 16 and _lib.CFM_TAP(7, 11) == 139
    for name in ("sylber_cfm_set_tap", "sylber_cfm_tap_floats", "sylber_cfm_tap_floats_packed"):
        assert name in _lib.DEV_EXPORTS and name not in _lib.EXPORTS
    assert lib.sylber_cfm_set_tap(None, 1, None, 0) != 0
    assert lib.sylber_cfm_tap_floats(None, 1, 1, 1) == -1 and lib.sylber_cfm_tap_floats_packed(None, 1, None, 1) == -1


def test_segment_scalars_aid_is_declared_on_both_sides(lib):
    """sylber_debug_segment_scalars (the segmenter's scalar chain for arrays of inputs, tests/test_gpu_segment_edges.py) is a development
    aid: declared in include/sylber_hip_dev.h with the signature the ctypes binding uses, exported, not part of the drop-in ABI, and its
    kernels live in segment.hip, the one source built without FMA contraction.  Host-only behaviour: bad counts and null arrays are refused
    before any launch."""
    from sylber_amd import _lib, build
    dev = open(os.path.join(ROOT, "include", "sylber_hip_dev.h")).read()
    m = re.search(r"int\s+sylber_debug_segment_scalars\s*\(([^)]*)\)", dev)
    assert m and [re.sub(r"\s+", " ", a.strip()) for a in m.group(1).split(",")] == [
        "const float* x_dev", "const float* d_dev", "int64_t n", "float* pow_dev", "float* sqrt_dev", "float* div_dev", "const float* c_dev",
        "const float* m_dev", "const int32_t* cnt_dev", "int64_t nwaves", "float* quot_dev", "void* stream"]
    assert "sylber_debug_segment_scalars" in _lib.DEV_EXPORTS and "sylber_debug_segment_scalars" not in _lib.EXPORTS
    assert len(_lib.DEV_EXPORTS["sylber_debug_segment_scalars"][1]) == 12 and hasattr(lib, "sylber_debug_segment_scalars")
    seg = open(os.path.join(ROOT, "sylber_amd", "csrc", "segment.hip")).read()
    assert 'extern "C" int sylber_debug_segment_scalars' in seg and build.EXTRA["segment.hip"] == ["-ffp-contract=off"]
    assert seg.count("merge_update(c, x, ") == 3              # the two scans and the aid run ONE merge update
    none = [None] * 3
    assert lib.sylber_debug_segment_scalars(None, None, -1, *none, *none, 0, None, None) != 0
    assert lib.sylber_debug_segment_scalars(None, None, 5, *none, *none, 0, None, None) != 0
    assert lib.sylber_debug_segment_scalars(None, None, 0, *none, *none, 3, None, None) != 0


def test_no_process_global_tuning_state():
    """tuning overrides are per handle (sylber_set_option) or per call: the old process-global force switches are gone"""
    for f in ("gemm_bf16.hip", "gemm_mxfp8.hip", "attention.hip", "api.hip", "forward.hip", "ops.hip", "ctx.h"):
        src = open(os.path.join(ROOT, "sylber_amd", "csrc", f)).read()
        assert "force_cfg" not in src and "g_force" not in src and "xpad_rows &" not in src, f


def test_num_frames_matches_conv_formula(lib):
    assert lib.sylber_num_frames(160000) == 499
    assert lib.sylber_num_frames(46080) == 143
    assert lib.sylber_num_frames(960000) == 2999
    assert lib.sylber_num_frames(400) == 1


def test_product_path_refuses_cpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from sylber_amd import Segmenter, _lib
    with pytest.raises(_lib.SylberHipError):
        Segmenter(model_ckpt=None)
    with pytest.raises(_lib.SylberHipError):
        Segmenter(model_ckpt=None, device="cpu")


def test_product_does_not_import_oracle():
    """The oracle is test infrastructure: nothing under sylber_amd/ may import it."""
    pkg = os.path.join(ROOT, "sylber_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, re.M), f
                assert "segment_ref" not in src and "hubert_ref" not in src, f


def test_bench_cli_parses():
    """bench.py's argument parser must build (a duplicated flag once broke the default run)"""
    import subprocess, sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--gpus" in r.stdout and "--steps" in r.stdout and "--warmup" in r.stdout


def test_no_packed_fp32_valu_in_the_library(lib):
    """v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 are banned from every kernel: beside MFMA waves of another kernel on
    the same SIMD they returned wrong values in lanes 48-63 (profiles/r02_packed_f32_hazard.md)"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import check_isa
    from sylber_amd import _lib
    text = check_isa.device_disassembly(_lib.LIB_PATH)                  # raises unless it really is the library's ISA
    n_dma = len(re.findall(r"\bbuffer_load_dwordx4\b[^\n]*\blds\b", text)) + len(re.findall(r"\bglobal_load_lds_dwordx4\b", text))
    assert len(re.findall(r"\bv_mfma_", text)) > 1000 and n_dma > 1000          # LDS-DMA staging (buffer descriptors since round 3)
    assert check_isa.banned_instructions(_lib.LIB_PATH) == {}


def test_ingest_rejects_rates_without_a_compact_resampling_table(lib):
    """host arithmetic only (no GPU): a corrupt WAVE header must not make the resampler plan a multi-GB polyphase table (a C++
    bad_alloc would cross the C ABI); common rates stay supported"""
    for sr, n16 in ((16000, 100000), (8000, 200000), (44100, 36282), (48000, 33334), (22050, 72563), (96000, 16667), (11025, 145125)):
        assert lib.sylber_ingest_num_frames(100000, sr) == n16 and lib.sylber_ingest_workspace_bytes(sr) > 0
    for sr in (0, -5, 44101, 15999, 2147483647):
        assert lib.sylber_ingest_num_frames(100000, sr) == -1 and lib.sylber_ingest_workspace_bytes(sr) == -1


def test_gemm_tile_cost_model_picks():
    """the tile cost model of the 16-bit GEMM launcher (csrc/gemm_bf16.hip TileModel) is host arithmetic: pinned here on the CPU tier so that an
    edit of its table cannot silently move the headline's kernels (round 6: a trailing comment once swallowed tile 91's row and FFN2 went to the
    256x256 four-wave tile, 0.73 -> 0.87 ms per forward).  Model 0 = the handle owns the chip, 5 = it shares it (two batches in flight)."""
    from sylber_amd import _lib
    lib = _lib.load()
    pick = lib.sylber_debug_gemm_pick
    QK, RESLN, BF16, GELU = 3, 6, 0, 1
    M = 32 * 512                                           # 32 x 10 s: 64 row tiles of 256
    # the headline batch: exactly 3 rounds (FFN1, q,k,v) / 1 round (out-proj, FFN2) of 256 tiles
    # (16-bit-output launches: the v_mfma_f32_16x16x32 family, the model offers ids 14 / 15 / 17 / 46 / 47; model + 100 = SYLBER_OPT_GEMM_MFMA16 -1, the 32x32x16 kernels)
    assert pick(M, 3072, 768, BF16, GELU, 0, 0, 0) == 47 and pick(M, 3072, 768, BF16, GELU, 0, 5, 0) == 47
    assert pick(M, 3072, 768, BF16, GELU, 0, 100, 0) == 97 and pick(M, 3072, 768, BF16, GELU, 0, 105, 0) == 97
    assert pick(M, 768, 3072, RESLN, 0, 0, 0, 0) == 91 and pick(M, 768, 3072, RESLN, 0, 0, 5, 0) == 91
    assert pick(M, 768, 768, RESLN, 0, 0, 0, 0) == 91 and pick(M, 768, 768, RESLN, 0, 0, 5, 0) == 91
    assert pick(M, 2304, 768, QK, 0, 0, 0, 0) == 4 and pick(M, 2304, 768, QK, 0, 0, 5, 0) == 91
    assert pick(M * 32, 512, 1536, BF16, GELU, 0, 0, 1) == 47          # conv1 in its chunk-major K order
    assert pick(M * 32, 512, 1536, BF16, GELU, 0, 100, 1) == 97        # (32x32x16 kernels: the only generated tile that has it)
    # 8 x 60 s (94 row tiles: 1.47 rounds of 256x192): alone on the chip the 192-row tile fills its second round, sharing it the round-5 choice stays
    ML = 8 * 3008
    assert pick(ML, 768, 3072, RESLN, 0, 0, 0, 0) == 51 and pick(ML, 768, 3072, RESLN, 0, 0, 5, 0) == 91
    assert pick(ML, 768, 768, RESLN, 0, 0, 0, 0) == 51
    assert pick(ML, 3072, 768, BF16, GELU, 0, 0, 0) == 47 and pick(ML, 3072, 768, BF16, GELU, 0, 100, 0) == 97
    assert pick(ML, 2304, 768, QK, 0, 0, 0, 0) == 4
    # 24 x 10 s (48 row tiles): 64 row tiles of 192 = exactly one round
    assert pick(24 * 512, 768, 3072, RESLN, 0, 0, 0, 0) == 51 and pick(24 * 512, 3072, 768, BF16, GELU, 0, 0, 0) == 46 and pick(24 * 512, 3072, 768, BF16, GELU, 0, 100, 0) == 57
    # small batches: 64-row tiles for the launches of one or two clips (fewer tiles than workgroup slots), not beyond (model + 6 = the round-6a choice)
    assert pick(512, 768, 3072, RESLN, 0, 0, 0, 0) == 1 and pick(512, 768, 768, RESLN, 0, 0, 0, 0) == 1 and pick(512, 2304, 768, QK, 0, 0, 0, 0) == 1
    assert pick(1024, 2304, 768, QK, 0, 0, 0, 0) == 2 and pick(2048, 768, 3072, RESLN, 0, 0, 0, 0) == 1 and pick(2048, 2304, 768, QK, 0, 0, 0, 0) == 3
    assert pick(512, 768, 3072, RESLN, 0, 0, 6, 0) == 51 and pick(8192, 768, 3072, RESLN, 0, 0, 0, 0) == 3
    # small batches of the 16-bit-output role: the 128x128 tile on eight waves
    assert pick(1024, 3072, 768, BF16, GELU, 0, 0, 0) == 15 and pick(8192, 512, 1536, BF16, GELU, 0, 0, 1) == 15 and pick(512, 3072, 768, BF16, GELU, 0, 100, 0) in (1, 2, 3, 4)
    # ... and its 64x64 three-slot form where a launch has at most ~one tile per workgroup slot (the conv layers of one or two clips)
    assert pick(2048, 512, 1536, BF16, GELU, 0, 0, 1) == 17 and pick(1024, 512, 1024, BF16, GELU, 0, 0, 0) == 17 and pick(512, 3072, 768, BF16, GELU, 0, 0, 0) == 17
    assert pick(2048, 512, 1536, BF16, GELU, 0, 6, 1) == 47
    # fp16 has the same tiles for the epilogues its forward launches
    assert pick(M, 768, 3072, RESLN, 0, 1, 0, 0) == 91 and pick(ML, 768, 3072, RESLN, 0, 1, 0, 0) == 51
    # every answer is a tile id that exists
    for m in (256, 1000, 6144, 12288, 16384, 24064, 49152):
        for (n, k, e, a) in ((2304, 768, QK, 0), (768, 768, RESLN, 0), (3072, 768, BF16, GELU), (768, 3072, RESLN, 0), (512, 1024, BF16, GELU)):
            for model in (0, 5, 100, 105):
                ids = (14, 15, 17, 46, 47) if (e == BF16 and model < 100) else (1, 2, 3, 4, 10, 85, 91, 97, 86, 51, 57, 80, 90, 95)
                assert pick(m, n, k, e, a, 0, model, 0) in ids, (m, n, k, e, model)


# ---- which kernel instantiation every launch of the 16-bit GEMM launcher resolves to (sylber_debug_gemm_resolve; host arithmetic only) ----
GEMM_DISPATCH_FIXTURE = os.path.join(ROOT, "tests", "golden", "gemm_dispatch.txt")
_FORCED_IDS = list(range(-1, 100)) + [9010]                 # 9010 = tile 10 with one workgroup per tile (never its persistent form)
_EPI_ACTS = ((0, 0), (0, 1), (0, 2), (0, 3), (1, 0), (1, 1), (1, 2), (2, 0), (6, 0), (3, 0), (4, 0))   # every epilogue of launch_gemm_bf16 with its activations


def _gemm_dispatch_grid():
    """the grid as (line key, [arguments of sylber_debug_gemm_resolve without the buffer]): M N K epi act fmt kpat tile model h192 pre tail.
    Forced cross: a line = one launch under every forced id (N = 1536: whole 192- and 256-column tiles and more than one round at M = 16384, so
    that tile 91's residual prefetch and tile 10's persistent form are reachable).  Automatic pick: a line = one launch."""
    for epi, act in _EPI_ACTS:
        for fmt in (0, 1, 2):
            for K, N, kpat in [(k, 1536, 0) for k in (64, 128, 192, 256, 768, 1536, 3072)] + [(1536, 512, 1)]:
                for mfma16 in (0, 1000000):
                    for M in (1000, 16384):
                        key = "forced %d %d %d %d %d %d %d %d" % (M, N, K, epi, act, fmt, kpat, mfma16)
                        yield key, [(M, N, K, epi, act, fmt, kpat, (mfma16 + t) if t >= 0 else (mfma16 + 999 if mfma16 else -1), 0, 0, 0, 0) for t in _FORCED_IDS]
    QK, RESLN, BF16, GELU = 3, 6, 0, 1
    rows = ((2304, 768, QK, 0, 0), (768, 768, RESLN, 0, 0), (3072, 768, BF16, GELU, 0), (768, 3072, RESLN, 0, 0), (512, 1024, BF16, GELU, 0), (512, 1536, BF16, GELU, 1))
    for M in (256, 512, 1000, 1024, 2048, 6144, 8192, 12288, 16384, 24064, 49152):
        for N, K, epi, act, kpat in rows:
            for model in (0, 2, 5, 6):
                for h192 in (0, -1):
                    for pre in ((-1, 0, 1, 2, 3) if epi == RESLN else (0,)):
                        for tile in ((-1, 1000999) if epi == BF16 else (-1,)):
                            yield "auto %d %d %d %d %d %d %d %d %d %d" % (M, N, K, epi, act, kpat, tile, model, h192, pre), [(M, N, K, epi, act, 0, kpat, tile, model, h192, pre, 0)]
    # forced row splits (8 x 60 s, 1.47 rounds of tile 91: its full round on 91, the rest on 128x128 / 128x192), and one the model refuses
    for tile, tail in ((91, 4), (91, 5), (-1, 4), (3, 4)):
        yield "tail %d %d" % (tile, tail), [(24064, 768, 3072, RESLN, 0, 0, 0, tile, 0, 0, 0, tail)]


def _gemm_dispatch_results(lib, intern):
    """[(key, [result per case])]: a result = the interned kernel name of the launch, `first-end:name` per launch of a row split, `x` = refused"""
    import ctypes
    buf = ctypes.create_string_buffer(4096)
    out = []
    for key, cases in _gemm_dispatch_grid():
        res = []
        for c in cases:
            n = lib.sylber_debug_gemm_resolve(*c, buf, len(buf))
            assert n >= 0, (key, c)
            launches = [ln.split(" ", 2) for ln in buf.value.decode().splitlines()] if n else []
            assert len(launches) == n
            if n == 1 and (int(launches[0][0]), int(launches[0][1])) == (0, c[0]):
                res.append(intern(launches[0][2]))
            else:
                res.append("+".join("%s-%s:%s" % (m0, m1, intern(nm)) for m0, m1, nm in launches) or "x")
        out.append((key, res))
    return out


def _rle(res):
    runs = []
    for r in res:
        if runs and runs[-1][0] == r:
            runs[-1][1] += 1
        else:
            runs.append([r, 1])
    return " ".join(r if n == 1 else "%s*%d" % (r, n) for r, n in runs)


def test_gemm_dispatch_resolves_to_the_recorded_kernels(lib):
    """Every tile of a family returns the same bits by design, so a launch routed to the wrong member passes every parity test and only runs slower:
    the routing is pinned here.  tests/golden/gemm_dispatch.txt holds, for a grid of launches (_gemm_dispatch_grid), the kernel instantiation(s)
    launch_gemm_bf16 resolved each to BEFORE the dispatch became one resolver per kernel family (recorded from the launch wrappers of that tree run
    dry), except forced ids without an instantiation, which since then take the documented 128x192 fallback uniformly.
    File: `name <index> <kernel>` lines, then `<key> | <results, run-length encoded>` lines."""
    names, want = {}, {}
    for ln in open(GEMM_DISPATCH_FIXTURE).read().splitlines():
        if ln.startswith("name "):
            _, idx, nm = ln.split(" ", 2)
            names[nm] = idx
        elif ln and not ln.startswith("#"):
            key, res = ln.split(" | ")
            want[key] = res
    got = _gemm_dispatch_results(lib, lambda nm: names.get(nm, "<" + nm + ">"))
    assert [k for k, _ in got] == list(want), "the grid and the fixture list different launches"
    bad = [(k, _rle(r), want[k]) for k, r in got if _rle(r) != want[k]]
    assert not bad, "%d launches resolve to other kernels than recorded, e.g. %s: got %s, recorded %s" % ((len(bad),) + bad[0])
