"""Host-side pieces of the product (no GPU): the C-ABI library loads, exports
every declared symbol, and its M-step arithmetic equals the oracle's."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest
from scipy.special import digamma

import lc_oracle as o
from libcluster_amd import capi

ROOT = Path(__file__).resolve().parents[1]


def test_library_exports_every_declared_symbol(lib):
    names = capi.declared_symbols()
    assert len(names) >= 35
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/libcluster_hip.h but not exported"


def test_library_leaves_no_cxx_template_member_undefined():
    """Round 6 found hipcc's host pass leaving std::vector members undefined in the object when a multiversioned
    (target_clones) function instantiates them -- a shared library links anyway and fails at the first call.  Nothing of
    the C++ library's templates may be an undefined dynamic symbol of the built libraries."""
    import subprocess

    for name in ("libcluster_hip.so", "libcluster_hip_testhooks.so"):
        r = subprocess.run(["nm", "-D", "-u", "-C", str(ROOT / "libcluster_amd" / "lib" / name)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        bad = [ln for ln in r.stdout.splitlines() if "std::vector<" in ln or "__normal_iterator<" in ln or "_Vector_base<" in ln]
        assert not bad, (name, bad)


def test_test_hooks_live_in_the_hooks_library_only(lib):
    """The lc_test_* entry points (csrc/lc_testhooks.hip: single launchers on host arrays, tests/test_gpu_aux_kernels.py)
    are linked into libcluster_hip_testhooks.so only: the shipped library exports none of them, the hooks library every
    one the Python helper declares -- and otherwise the same symbols as the shipped one.  (Both load without a GPU.)"""
    import aux_hooks

    shipped = aux_hooks.exported_symbols(aux_hooks.SHIPPED_LIB)
    hooked = aux_hooks.exported_symbols(aux_hooks.HOOKS_LIB)
    assert not [s for s in shipped if s.startswith("lc_test_")]
    declared = set(aux_hooks.PROTOTYPES)
    assert len(declared) >= 27 and declared <= hooked, sorted(declared - hooked)
    # the launchers of lc_kernels_diag.hip (tests/test_gpu_diag_kernels.py) and the host packer of their matrix-pipe operands
    assert {"lc_test_estep_diag_plan", "lc_test_estep_diag", "lc_test_suffstat_diag_plan", "lc_test_suffstat_diag", "lc_test_diag_pack",
            "lc_test_diag_weights"} <= declared and len(declared) >= 41
    assert {s for s in hooked if s.startswith("lc_test_")} == declared  # no hook without a prototype either
    assert {s for s in shipped if s.startswith("lc_")} == {s for s in hooked if s.startswith("lc_")} - declared
    h = aux_hooks.hooks()  # loads, and every prototype binds
    assert all(hasattr(h, n) for n in declared)


def test_aux_hooks_constants_are_those_of_the_sources():
    """tests/aux_hooks.py restates the constants that decide which path a launcher takes; the cases of
    tests/test_gpu_aux_kernels.py sit on both sides of them."""
    import re

    import aux_hooks

    csrc = ROOT / "libcluster_amd" / "csrc"
    text = "".join((csrc / f).read_text() for f in ("lc_kernels.h", "lc_device.hpp", "lc_kernels_aux.hip"))

    def const(name):
        m = re.findall(r"\b" + name + r"\s*=\s*(?:\(int64_t\))?(0x[0-9A-Fa-f]+|\d+)", text)
        assert len(m) == 1, (name, m)
        return int(m[0], 0)

    for name in ("REDUCE_TMP_ELEMS", "SEL_ROWS", "GCS_SLICES", "BOUND_MAX_COLS", "BOUND_MAX_K", "QHASH_SEED", "SS_BR"):
        assert const(name) == getattr(aux_hooks, name), name
    assert "enum SuffstatRoute { SS_PER_CLUSTER = 0, SS_FEAT = 1, SS_QUAD = 2, SS_WIDE = 3 };" in text
    assert "enum SuffstatMode { SS_DENSE = 0, SS_MASKED_DENSE = 1, SS_ZERO_SKIP = 2, SS_WORK_LIST = 3 };" in text
    assert const("QHASH_NONE") - (1 << 64) == aux_hooks.QHASH_NONE
    assert "if (tmp && nparts > 8192 && n <= REDUCE_TMP_ELEMS)" in text and "nparts > 512 && n <= 4096" in text
    assert "rows >= (int64_t)J * 65536" in text and "if (J > 1024)" in text  # the boundaries the test file names
    # the prediction and document-inference kernels (tests/test_gpu_predict_kernels.py)
    text = "".join((csrc / f).read_text() for f in ("lc_predict.hpp", "lc_kernels.h", "lc_kernels_topic.hip", "lc_kernels_predict.hip"))
    for name in ("PR_COLS", "PC_CHUNK", "PC_PANEL", "PC_WAVE_ROWS", "PC_THREADS", "PRED_RENORM", "TI_KR", "TOPIC_E_LDS"):
        assert const(name) == getattr(aux_hooks, name), name
    assert "TOPIC_LDS_BYTES = 40 * 1024;" in text and aux_hooks.TOPIC_LDS_BYTES == 40 * 1024
    assert "for (int k0 = 0; k0 < Kmax; k0 += PR_COLS)" in text and "const int Kmax = a.K > a.Kp ? a.K : a.Kp;" in text
    assert "if (a.K <= TI_KR)" in text and "if (N * K <= a.tile_cap)" in text  # registers or not; tile in LDS or not
    assert "(int64_t)T * K <= TOPIC_E_LDS ? 1 : 0" in text
    for dp in (16, 32, 48, 64):  # the register-resident instances of predict_diag_kernel; every other width is generic
        assert text.count(f"case {dp}: hipLaunchKernelGGL((predict_diag_kernel<MODE, {dp}>)") == 1
    assert "default: hipLaunchKernelGGL((predict_diag_kernel<MODE, 0>)" in text
    assert "a.DP % PRED_RENORM != 0" in text
    assert "x[g][s] = c < a.Da ? a.X[(size_t)xrow[g] * a.DP + c] : c == a.Da ? 1.0 : 0.0;" in text  # the ones column
    # the hot path (tests/test_gpu_hot_kernels.py): tile and table sizes of the fused pass, the instances of the E-step
    text = "".join((csrc / f).read_text() for f in ("lc_kernels.h", "lc_kernels_fused.hip", "lc_kernels_estep.hip"))
    for name in ("FUSED_ROWS", "FUSED_KMAX", "FUSED_CT_CAP", "SS_BR"):
        assert const(name) == getattr(aux_hooks, name), name
    assert "constexpr int WIDE_R = 2, WIDE_WAVES = 4;" in text and (aux_hooks.WIDE_R, aux_hooks.WIDE_WAVES) == (2, 4)
    assert "constexpr int WIDE_CHUNK = 256 * 16 + 64;" in text and aux_hooks.WIDE_CHUNK == 256 * 16 + 64
    assert "constexpr size_t ES_LQ_LDS_CAP = 80 * 1024;" in text and aux_hooks.ES_LQ_LDS_CAP == 80 * 1024
    assert "constexpr int estep_cfg_r(int DP) { return DP <= 48 ? 4 : DP <= 96 ? 3 : 2; }" in text
    assert "constexpr int estep_cfg_waves(int DP) { return DP <= 96 ? 4 : 8; }" in text
    assert [aux_hooks.estep_cfg_r(d) for d in (16, 48, 64, 96, 112, 128)] == [4, 4, 3, 3, 2, 2]
    assert [aux_hooks.estep_cfg_waves(d) for d in (16, 96, 112, 128)] == [4, 4, 8, 8]
    assert 'atoi(test_switch("LC_FUSED_YSHARE")) : 410;' in text and aux_hooks.FUSED_YSHARE == 410
    assert "a.yshare = a.grid == 2 * cus ? ys : 0;" in text
    assert "(DP == 64 || DP == 80) && !a.sparse && a.K >= 6 && lq_fits(4, 4)" in text  # K = 6: where the four-row-group instance starts
    # the separable families (tests/test_gpu_diag_kernels.py, tests/diag_refs.py): tile counts, caps and LDS limits of lc_kernels_diag.hip
    import diag_refs

    text = "".join((csrc / f).read_text() for f in ("lc_kernels.h", "lc_kernels_diag.hip"))
    for name in ("DIAG_MAXT", "SD_QMAX", "EDM_CT_CAP", "EDM_KTM"):
        assert const(name) == getattr(diag_refs, name), name
    assert "constexpr size_t EDM_LDS_LIMIT = 150 * 1024;" in text and diag_refs.EDM_LDS_LIMIT == 150 * 1024
    assert "constexpr size_t EDM_LDS_TWO_BLOCKS = 80 * 1024;" in text and diag_refs.EDM_LDS_TWO_BLOCKS == 80 * 1024
    assert "p.per_cu = p.lds_bytes <= EDM_LDS_TWO_BLOCKS ? 2 : 1;" in text
    assert "if (edm_lds_bytes(NT, NTF, KT, R, K > 4 * EDM_KTM) > EDM_LDS_LIMIT) return 0;" in text
    assert "constexpr int edm_r(int NT) { return NT <= 16 ? 2 : 1; }" in text  # R = NT <= 16 ? 2 : 1
    assert [diag_refs.edm_r(nt) for nt in (4, 16, 20, 32)] == [2, 2, 1, 1]
    assert "constexpr int sd_br(int DP) { return DP <= 64 ? 32 : 16; }" in text and (diag_refs.sd_br(64), diag_refs.sd_br(80)) == (32, 16)
    assert "constexpr bool sd_nstage(int DP, int RS) { return DP <= 96 && !(DP >= 64 && RS == 1); }" in text
    assert "constexpr bool sd_deep(int DP) { return DP <= 96; }" in text
    assert "p.KT = a.K <= 4 ? 1 : a.K <= 8 ? 2 : 4;" in text and "p.REG = a.K <= 4 * DIAG_MAXT * 4;" in text
    assert "enum DiagEstepInstance { EDI_NONE = 0, EDI_GENERIC = 1, EDI_PLAIN = 2, EDI_TABLED = 3, EDI_ONEGROUP = 4 };" in text
    assert diag_refs.EDI == aux_hooks.EDI_NAMES == ("none", "generic", "plain", "tabled", "one_group")
    assert "constexpr int DIAG_SINK = 256, DIAG_SINK_GUARD = 64;" in (csrc / "lc_testhooks.hip").read_text()
    assert (aux_hooks.DIAG_SINK, aux_hooks.DIAG_SINK_GUARD) == (256, 64)
    # the workgroup size the API picks, which lc_test_topic_infer restates for threads = 0
    pick = "maxN <= 64 ? 64 : maxN <= 128 ? 128 : 256;"
    assert pick in (csrc / "lc_topic_predict.cpp").read_text() and pick in (csrc / "lc_testhooks.hip").read_text()


def test_constants(lib):
    assert lib.lc_const_converge() == o.CONVERGE
    assert lib.lc_const_fengydel() == o.FENGYDEL
    assert lib.lc_const_zerocutoff() == o.ZEROCUTOFF
    assert lib.lc_const_splititer() == o.SPLITITER


def test_digamma_matches_scipy(lib):
    x = np.concatenate([np.linspace(1e-3, 12, 2000), np.logspace(1, 8, 200), [0.5, 1.0, 1.4616321449683623, 60.5]])
    got = np.array([lib.lc_digamma(float(v)) for v in x])
    ref = digamma(x)
    assert np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref))) < 5e-15
    # NaN in, NaN out (an all-inactive group in sparse mode produces NaN counts; this used to recurse forever);
    # negative non-integers through the reflection formula; poles give NaN at this C entry point
    assert np.isnan(lib.lc_digamma(float("nan")))
    for v in (-0.5, -1.25, -7.75):
        assert abs(lib.lc_digamma(v) - digamma(v)) < 1e-12 * max(1.0, abs(digamma(v)))
    assert np.isnan(lib.lc_digamma(0.0)) and np.isnan(lib.lc_digamma(-3.0))
    assert lib.lc_digamma(float("inf")) == float("inf")


@pytest.mark.parametrize("kind,cls", [(capi.W_DIRICHLET, o.Dirichlet), (capi.W_STICKBREAK, o.StickBreak),
                                      (capi.W_GDIRICHLET, o.GDirichlet)])
def test_weights_update_matches_oracle(lib, kind, cls):
    rng = np.random.default_rng(3)
    for K in (1, 2, 5, 17):
        Nk = rng.uniform(0, 50, K)
        w = cls()
        w.update(Nk)
        e, f = capi.weights_update(kind, Nk)
        np.testing.assert_allclose(e, w.Elogweight(), rtol=1e-13, atol=1e-13)
        assert abs(f - w.fenergy()) <= 1e-12 * max(1.0, abs(w.fenergy()))
    if kind != capi.W_GDIRICHLET:
        w = cls(2.5)
        w.update(np.array([3.0, 9.0, 1.0]))
        e, f = capi.weights_update(kind, np.array([3.0, 9.0, 1.0]), 2.5)
        np.testing.assert_allclose(e, w.Elogweight(), rtol=1e-13)
        assert abs(f - w.fenergy()) < 1e-11


def test_gw_mstep_matches_golden(lib, estep_cases):
    for c in estep_cases:
        D, K = c["D"], c["K"]
        for k in range(K):
            r = capi.gw_mstep(c["prior"], c["stats"]["Nk"][k], np.array(c["stats"]["xs"][k]),
                              np.array(c["stats"]["xxs"][k]))
            p = c["post"]
            assert abs(r["nu"] - p["nu"][k]) < 1e-12 * p["nu"][k]
            assert abs(r["beta"] - p["beta"][k]) < 1e-12 * p["beta"][k]
            np.testing.assert_allclose(r["m"], p["m"][k], rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(r["iW"], np.array(p["iW"][k]), rtol=1e-11, atol=1e-10)
            assert abs(r["logdW"] - p["logdW"][k]) < 1e-10 * max(1, abs(p["logdW"][k]))
            assert abs(r["fenergy"] - p["Fc"][k]) < 1e-9 * max(1, abs(p["Fc"][k]))
            # whitener: nu * maha(x) == ||A (x - m)||^2
            x = np.array(c["X"][0][0])
            g = o.GaussWish(c["prior"], D)
            g.addstats(c["stats"]["Nk"][k], c["stats"]["xs"][k], c["stats"]["xxs"][k])
            g.update()
            lhs = g.nu * o.mahaldist(x[None, :], g.m, g.iW)[0]
            rhs = np.sum((r["A"] @ (x - r["m"])) ** 2)
            assert abs(lhs - rhs) < 1e-9 * max(1.0, lhs)
            assert abs((r["eloglike_const"] - 0.5 * rhs) - g.Eloglike(x[None, :])[0]) < 1e-9 * max(1.0, abs(lhs))


def test_error_mapping(lib):
    with pytest.raises(ValueError):
        capi.weights_update(capi.W_DIRICHLET, np.array([1.0]), wprior=0.0)  # "Alpha prior must be > 0!"
    with pytest.raises(ValueError):
        capi.gw_mstep(0.0, 1.0, np.zeros(2), np.eye(2))  # "clustwidth must be > 0!"
    with pytest.raises(RuntimeError):  # non-PD iW in update -> runtime_error (distributions.cpp:333-336)
        capi.gw_mstep(1.0, 5.0, np.zeros(2), -100 * np.eye(2))


def test_no_cpu_fallback(lib):
    """Without a GPU every data-path entry point must fail loudly."""
    if lib.lc_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(capi.HipError):
        capi.Context(0)
    with pytest.raises(capi.HipError):
        capi.learn(capi.ALGO_BGMM, np.zeros((4, 2)))


def test_ng_and_eg_mstep_match_oracle(lib):
    """NormGamma / ExpGamma update(), fenergy() and the Eloglike constant (distributions.cpp:441-464, 508-517,
    545-552, 584-589) against the oracle, incl. odd D (the reference's integer D/2 in NormGamma::fenergy)."""
    from scipy.special import digamma

    rng = np.random.default_rng(3)
    for D in (1, 2, 5, 16, 33):
        n = 40
        Xn = rng.normal(size=(n, D)) * 2 + 1
        q = rng.uniform(0.05, 1.0, n)
        for prior in (1.0, 0.3):
            c = o.NormGamma(prior, D)
            c.addobs(q, Xn)
            c.update()
            r = capi.ng_mstep(prior, q.sum(), q @ Xn, q @ (Xn * Xn))
            assert abs(r["nu"] - c.nu) < 1e-12 and abs(r["beta"] - c.beta) < 1e-12
            np.testing.assert_allclose(r["m"], c.m, rtol=1e-12, atol=1e-13)
            np.testing.assert_allclose(r["L"], c.L, rtol=1e-11)
            assert abs(r["logL"] - c.logL) < 1e-10
            assert abs(r["fenergy"] - c.fenergy()) < 1e-9 * max(1, abs(c.fenergy()))
            cst = 0.5 * (D * (digamma(c.nu) - np.log(2 * np.pi) - 1 / c.beta) - c.logL)
            assert abs(r["eloglike_const"] - cst) < 1e-10
            Xe = np.abs(Xn)
            e = o.ExpGamma(prior, D)
            e.addobs(q, Xe)
            e.update()
            r = capi.eg_mstep(prior, q.sum(), q @ Xe)
            assert abs(r["a"] - e.a) < 1e-12 and abs(r["logb"] - e.logb) < 1e-11
            np.testing.assert_allclose(r["ib"], e.ib, rtol=1e-12)
            assert abs(r["fenergy"] - e.fenergy()) < 1e-9 * max(1, abs(e.fenergy()))
            assert abs(r["eloglike_const"] - (D * digamma(e.a) - e.logb)) < 1e-10


def test_statistics_kernel_selection_is_a_function_of_the_shape(lib, monkeypatch):
    """lc_statistics_kernel_name (no device needed): the dense Gauss-Wishart statistics pass runs as the feature GEMM
    where it was measured to win (the widths with instances that do not spill; cluster counts whose remainder launch
    carries at least four clusters), as the per-cluster kernel elsewhere -- a property of (D, K) alone, so every rank of a sharded run takes the same kernel."""
    monkeypatch.delenv("LC_SS_FEAT", raising=False)
    fn = lib.lc_statistics_kernel_name
    fn.restype = C.c_char_p
    fn.argtypes = [C.c_int, C.c_int]
    feat, per = b"suffstat_feat_kernel", b"suffstat_kernel"
    assert fn(64, 32) == feat and fn(61, 30) == feat and fn(64, 28) == feat and fn(64, 64) == feat
    assert fn(128, 64) == feat and fn(32, 32) == feat and fn(48, 29) == feat
    # round 4 (chunk counts that fill the last round of resident blocks): at D <= 64 a remainder launch pays from four
    # clusters on; D = 128 takes 64 clusters in one pass for K mod 64 in {0, 57 ... 63}
    assert fn(64, 24) == feat and fn(64, 48) == feat and fn(64, 36) == feat and fn(32, 40) == feat
    assert fn(128, 60) == feat and fn(128, 128) == feat and fn(128, 121) == feat
    assert fn(128, 40) == per and fn(128, 48) == per
    assert fn(64, 33) == per and fn(64, 35) == per
    assert fn(80, 32) == feat and fn(96, 32) == feat and fn(112, 40) == feat and fn(96, 20) == feat   # (round 5: 8-wave blocks, no scratch)
    assert fn(96, 33) == per and fn(80, 12) == per and fn(96, 16) == feat
    assert fn(16, 32) == per and fn(256, 32) == per
    # round 6: up to 16 clusters at D = 17 ... 64 the four clusters of a quad ride in the four blocks of one MFMA
    quad = b"suffstat_quad_kernel"
    # (from three clusters on: the four blocks of a quad work whether their cluster exists or not, and K = 2 loses to that)
    for D, K in ((64, 8), (64, 16), (23, 16), (48, 12), (64, 4), (33, 7), (17, 11), (40, 15), (40, 3), (64, 6), (32, 14), (33, 9)):
        assert fn(D, K) == quad, (D, K)
    assert fn(64, 2) == per and fn(17, 1) == per
    assert fn(64, 17) == feat and fn(16, 8) == per and fn(80, 12) == per and fn(80, 16) == feat
    # ... and the feature GEMM skips the patches of the padding's idle columns (active width = D rounded up to 8, where that is
    # below the padded width): from five clusters on it is then the faster one at the wider layouts too
    assert fn(72, 8) == feat and fn(88, 6) == feat and fn(104, 12) == feat and fn(120, 5) == feat and fn(72, 4) == per
    assert fn(80, 8) == per and fn(96, 8) == per


def test_roofline_traffic_json_is_generated_from_the_committed_summaries():
    """bench.py's roofline.traffic comes from profiles/rNN_pmc_traffic.json; that file is the output of
    tools/pmc_traffic.py over the TRAFFIC lines of the rocprofv3 summaries committed next to it (round 3's table was
    maintained by hand and drifted from its profiles).  The newest JSON must be exactly what its summaries say, and
    every bench configuration with a summary of that round must be in it."""
    import json
    import re
    import subprocess
    import sys

    prof = ROOT / "profiles"
    files = sorted(prof.glob("r[0-9][0-9]_pmc_traffic.json"))
    assert files
    newest = files[-1]
    rnd = newest.name[:3]
    if int(rnd[1:]) < 4:
        pytest.skip("no generated traffic table yet (rounds 1-3 typed theirs)")
    r = subprocess.run([sys.executable, str(ROOT / "tools" / "pmc_traffic.py"), rnd, "--check"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    d = json.loads(newest.read_text())
    for f in prof.glob(f"{rnd}_*_rocprof_summary.txt"):
        line = [ln for ln in f.read_text().splitlines() if ln.startswith("TRAFFIC ")]
        if not line:
            continue
        inst = json.loads(line[-1][8:])
        users = [k for k, v in d.items() if isinstance(v, dict) and v.get("_summary") == f.name]
        assert users, f.name
        for name, e in inst.items():
            fam = name.split("<")[0]
            # the same number the human-readable part of the summary prints (GB per launch, three decimals)
            txt = f.read_text()
            m = re.search(re.escape("[" + name + "]") + r".*?HBM read\s+\(FETCH_SIZE\*1024\*2\)\s+([0-9.]+) GB", txt, re.S)
            if m:
                assert abs(float(m.group(1)) * 1e9 - e["read_bytes"]) <= 6e5, (name, m.group(1), e)
            assert any(fam in d[u] for u in users)


def test_estep_kernel_isa_keeps_the_promises_its_inline_asm_relies_on():
    """estep_kernel writes M0 and loads c_jk in inline asm that hipcc's waitcnt pass cannot see (lc_kernels_estep.hip);
    tools/check_isa.py compiles the device code and asserts on the ISA of every instance: no scratch, M0 named only by
    the LDS-direct load pairs, nothing touching an asm load's destination before its s_waitcnt vmcnt(0); and, over the
    estep / fused / diag kernels, no inline-asm statement reading an MFMA result inside the MFMA's hazard window (the
    compiler does not count wait states for asm: the round-4 NaN rows of the half-width fused instance)."""
    import subprocess
    import sys

    r = subprocess.run([sys.executable, str(ROOT / "tools" / "check_isa.py")], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "estep_kernel instances: ok" in r.stdout
    assert "inline-asm statements behind MFMAs in 3 files: ok" in r.stdout


def test_isa_checker_sees_an_asm_read_inside_an_mfma_hazard_window():
    """The checker itself, on assembly written for the purpose: an inline-asm v_max_f64 that reads an accumulator three
    instructions behind the MFMA that wrote it is reported; the same read behind a compiler-generated instruction that
    overwrote the register, or far enough behind the MFMA, is not."""
    import importlib.util

    spec = importlib.util.spec_from_file_location("check_isa", ROOT / "tools" / "check_isa.py")
    ci = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ci)
    head = "_Z4kernv: ; @kern\n"
    tail = "\n.Lfunc_end0:\n"
    bad = head + """	v_mfma_f64_4x4x4_4b_f64 v[10:11], v[2:3], v[4:5], v[10:11]
	s_nop 1
	;;#ASMSTART
	v_max_f64 v[20:21], v[20:21], v[10:11]
	;;#ASMEND""" + tail
    problems, nasm = ci.check_mfma_into_asm(bad)
    assert nasm == 1 and len(problems) == 1 and "v[10, 11]" in problems[0]
    rewritten = head + """	v_mfma_f64_4x4x4_4b_f64 v[10:11], v[2:3], v[4:5], v[10:11]
	v_max_f64 v[10:11], v[10:11], v[10:11]
	;;#ASMSTART
	v_max_f64 v[20:21], v[20:21], v[10:11]
	;;#ASMEND""" + tail
    assert ci.check_mfma_into_asm(rewritten) == ([], 1)
    far = head + "\tv_mfma_f64_4x4x4_4b_f64 v[10:11], v[2:3], v[4:5], v[10:11]\n" + "\ts_nop 7\n" * 3 + """	;;#ASMSTART
	v_max_f64 v[20:21], v[20:21], v[10:11]
	;;#ASMEND""" + tail
    assert ci.check_mfma_into_asm(far) == ([], 1)


def test_blocked_host_factorisations_are_bit_identical_to_the_element_by_element_forms(tmp_path):
    """tests/cpp/host_linalg_test.cpp: the M-step's Cholesky and triangular inverse (4 x 4 blocks, four-row-interleaved
    factor, AVX2 clone where the CPU has it) against the textbook loops with the same order of operations per element, n = 1
    ... 150, by memcmp -- with g++ and with the compiler the library is built with."""
    import shutil
    import subprocess

    src = ROOT / "tests" / "cpp" / "host_linalg_test.cpp"
    compilers = [["g++", "-O2"]]
    if shutil.which("/opt/rocm/lib/llvm/bin/clang++"):
        compilers.append(["/opt/rocm/lib/llvm/bin/clang++", "-O3"])
    for i, cc in enumerate(compilers):
        exe = tmp_path / f"host_linalg_{i}"
        r = subprocess.run([*cc, "-std=c++17", "-Wall", f"-I{ROOT / 'include'}", f"-I{ROOT / 'libcluster_amd' / 'csrc'}", str(src), "-o",
                            str(exe)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0 and "bit-identical" in r.stdout, r.stdout + r.stderr
