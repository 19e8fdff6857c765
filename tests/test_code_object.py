"""CPU-side checks of the built libraries' device code (no GPU needed), each made once for every library of
``kernel_census.LIBRARIES``: gfx950 code objects only (tests/code_object.py reads them), every kernel's register / LDS budget
inside the CU's limits, no kernel spills registers to scratch memory, the five libraries share no kernel name, and the census
rules of tests/kernel_census.py on every library that has a fixture.  What is specific to one kernel family -- instance counts,
exact key sets, tighter budgets -- is in that family's host test."""
import functools
import os

import pytest

import kernel_census as census
from code_object import LIB, _code_objects
from golden_util import ROOT

NAMES = sorted(census.LIBRARIES)
WITH_FIXTURE = [n for n in NAMES if census.LIBRARIES[n].fixture]
# 14 kernels of the main library (conv_halo_dw, two conv_halo_ws rings, detect_kernel among them) keep some SGPRs in VGPR lanes --
# ``.sgpr_spill_count`` up to 87, no scratch memory --, as they did before this count was looked at; no other library does
SGPR_SPILLS = ("main",)


@functools.lru_cache(maxsize=None)
def _kernels(name):
    return census.kernels(name)           # (asserts: built, device code for gfx950 only)


@pytest.fixture(scope="module")
def kernels():
    return _kernels("main")


def test_library_has_the_hot_path_kernels(kernels):
    names = " ".join(k[".name"] for k in kernels)
    for needle in ("conv_halo_ws_kernel", "conv_patch_wsp_kernel", "conv_igemm2_kernel", "conv_igemm3_kernel",
                   "conv_stem_s2_fused_kernel", "conv_resblock_fused_kernel", "yolo_decode_kernel", "detect_kernel",
                   "pack_records_kernel", "resize"):
        assert needle in names, needle


@pytest.mark.parametrize("name", NAMES)
def test_no_kernel_spills_and_budgets_fit_a_cu(name):
    """no scratch, no spilled VGPR (nor SGPR, the main library aside), at most 512 VGPR + AGPR, at most 160 KiB of static LDS,
    wave64"""
    assert _kernels(name)
    for k in _kernels(name):
        sym = k[".name"]
        assert k[".private_segment_fixed_size"] == 0, (sym, "uses scratch memory (register spills)")
        assert k[".vgpr_spill_count"] == 0, sym
        assert name in SGPR_SPILLS or k[".sgpr_spill_count"] == 0, sym
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 512, sym
        assert k[".group_segment_fixed_size"] <= 160 * 1024, sym
        assert k[".wavefront_size"] == 64, sym


def test_no_two_libraries_hold_a_kernel_of_the_same_name():
    """each library's device code is its own: a kernel family that moved into a library of its own is in no other, so no census
    (and not the device-code hash of the main library) sees another library's kernels"""
    names = {n: {k[".name"] for k in _kernels(n)} for n in NAMES}
    for i, a in enumerate(NAMES):
        for b in NAMES[i + 1:]:
            assert not names[a] & names[b], (a, b, sorted(names[a] & names[b]))


def test_device_code_hash_does_not_depend_on_the_build_directory(tmp_path):
    """bench.py ties profiles/r0N_traffic.json to the library by a hash over its DEVICE code.  hipcc embeds an id derived
    from the source path in every code object's symbol tables; the hash must not see it: one source
    compiled into two directories, under two different source paths, hashes the same -- and the raw objects do differ."""
    import shutil
    import subprocess
    import sys
    sys.path.insert(0, ROOT)
    import bench
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    csrc = os.path.join(ROOT, "pytorch-yolov3_amd", "csrc")
    objs = []
    for sub in ("a", os.path.join("b", "deeper")):
        d = tmp_path / sub
        d.mkdir(parents=True)
        for name in ("yolo_decode.hip", "common.h", "decode_core.h"):
            shutil.copy(os.path.join(csrc, name), str(d / name))
        out = str(d / "yolo_decode.o")
        subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"),
                               "-ffp-contract=off", "-Wno-unused-function", "-c", str(d / "yolo_decode.hip"), "-o", out])
        objs.append(out)
    raw = [open(o, "rb").read() for o in objs]
    code = [[elf for _, elf in _code_objects(r)] for r in raw]
    assert code[0] != code[1], "expected the path-derived id to differ between the two builds"
    assert bench.device_code_sha256(objs[0]) == bench.device_code_sha256(objs[1])
    # ... and it is a hash of the kernels: another source gives another value
    assert bench.device_code_sha256(objs[0]) != bench.device_code_sha256(LIB)


# ---- the census of compiled instances (tests/kernel_census.py), per library that keeps one -------------------------------------

def _census(name):
    if not os.path.exists(census.fixture_path(name)):
        pytest.fail("tests/golden/%s is missing (tools/make_kernel_instances.py --library %s writes it on an MI355X)" % (
            census.LIBRARIES[name].fixture, name))
    return census.load(name), {k[".name"] for k in _kernels(name)}


def _broken(name, fixture, library, *rules):
    return "\n".join(m for m in census.failures(name, fixture, library) if any(census.WHAT[r] in m for r in rules))


@pytest.mark.parametrize("name", WITH_FIXTURE)
def test_every_compiled_kernel_is_launched_by_a_footprint_case_or_provably_by_nothing(name):
    """Coverage: every ``.name`` of the library's code objects is in the union of the fixture's ``footprint`` map -- a one-op
    test with the oracle gate, the strided / poisoned run and the byte-for-byte footprint check launched it on an MI355X --
    or among the library's ``unreachable`` symbols with the chooser condition that excludes it.  Never both: no recorded GPU
    test launches an unreachable symbol."""
    fixture, library = _census(name)
    t = census.totals(name, fixture, library)
    print("%s kernel census: %s" % (name, census.summary(name, fixture, library)))
    rep = census.report(name, fixture, library)
    assert not rep["uncovered"] and not rep["unreachable_but_launched"], _broken(name, fixture, library, "uncovered", "unreachable_but_launched")
    assert t["covered"] + t["unreachable"] == t["symbols"]
    for sym, reason in census.LIBRARIES[name].unreachable.items():
        assert ".hip:" in reason, "UNREACHABLE[%s] names no chooser line" % sym


@pytest.mark.parametrize("name", WITH_FIXTURE)
def test_census_names_no_kernel_the_library_lacks(name):
    """Stale check: every symbol named in the fixture or as unreachable exists in the library (a removed or renamed instance
    must leave the record too).  The fixture holds a footprint table and, where the library has run-ahead kernels, a contention
    table, both filled; every symbol list is sorted, without repeats and not empty."""
    fixture, library = _census(name)
    assert not census.report(name, fixture, library)["stale"], _broken(name, fixture, library, "stale")
    assert set(fixture) <= {"footprint", "contention"} and fixture["footprint"]
    assert fixture.get("contention") or not census.LIBRARIES[name].run_ahead
    for table in fixture.values():
        for key, syms in table.items():
            assert syms == sorted(set(syms)) and syms, key


@pytest.mark.parametrize("name", WITH_FIXTURE)
def test_every_run_ahead_instance_runs_beside_the_copy_kernel(name):
    """Contention: every instance of the library's run-ahead families -- in the main library conv1x1_dw_kernel with both HEAD
    values, conv_dw48_kernel, conv_halo_dw_kernel: the kernels whose template parameter sets their wait counts; in the block
    library every kernel -- is in the union of the fixture's ``contention`` map, or unreachable."""
    fixture, library = _census(name)
    t = census.totals(name, fixture, library)
    if name == "main":
        assert t["run_ahead"] >= 2 * (9 + 5 + 14 + 3), t          # (both 16-bit types of the y3_ints lists as they stand)
    if name == "block":
        assert t["run_ahead"] == t["symbols"] > 0, t
    assert not census.report(name, fixture, library)["not_under_contention"], _broken(name, fixture, library, "not_under_contention")


def test_census_report_rules_on_hand_made_dictionaries(monkeypatch):
    """each of the four rules fires alone; "every kernel is run-ahead" works; a fixture without a contention table reads as one
    with an empty table"""
    ahead, plain, dead, gone = "_Z9ra_kernelILi1EEvv", "_Z5plainv", "_Z4deadv", "_Z4gonev"
    monkeypatch.setitem(census.LIBRARIES, "some", census.Library("some.so", None, ("ra_kernel",), {dead: "x.hip:1 never"}))
    monkeypatch.setitem(census.LIBRARIES, "all", census.Library("all.so", None, census.EVERY_KERNEL, {}))
    monkeypatch.setitem(census.LIBRARIES, "none", census.Library("none.so", None, (), {}))
    library = {ahead, plain, dead}

    def broken(name, footprint, contention, library=library):
        fixture = {"footprint": footprint} if contention is None else {"footprint": footprint, "contention": contention}
        rep = census.report(name, fixture, library)
        assert set(rep) == set(census.WHAT)
        assert len(census.failures(name, fixture, library)) == sum(1 for v in rep.values() if v)
        return {k: v for k, v in rep.items() if v}
    foot, cont = {"a": [ahead], "b": [plain]}, {"a": [ahead]}
    assert broken("some", foot, cont) == {}
    assert census.totals("some", {"footprint": foot, "contention": cont}, library) == {
        "symbols": 3, "covered": 2, "unreachable": 1, "run_ahead": 1, "under_contention": 1}
    assert broken("some", {"a": [ahead]}, cont) == {"uncovered": [plain]}
    assert broken("some", {"a": [ahead], "b": [dead, plain]}, cont) == {"unreachable_but_launched": [dead]}
    assert broken("some", dict(foot, c=[gone]), cont) == {"stale": [gone]}
    assert broken("some", foot, cont, library - {dead}) == {"stale": [dead]}
    assert broken("some", foot, {}) == broken("some", foot, None) == {"not_under_contention": [ahead]}
    # every kernel run-ahead: the kernel no contention case launches is named, whatever template it is an instance of
    assert broken("all", foot, cont, {ahead, plain}) == {"not_under_contention": [plain]}
    assert broken("all", foot, foot, {ahead, plain}) == {}
    # no run-ahead family: no contention table is needed, absent or empty
    assert broken("none", foot, None, {ahead, plain}) == broken("none", foot, {}, {ahead, plain}) == {}
    assert broken("none", {"a": [ahead]}, None, {ahead, plain}) == {"uncovered": [plain]}


def test_launch_log_entry_points_and_names(kernels):
    """``y3_debug_launch_log_begin`` / ``_end`` without a GPU: one log per thread, the size query leaves the log open, and the name
    logged for a launch is a ``.name`` of the code objects -- the log is written BEFORE the launch, which here fails for want of
    a device."""
    import ctypes

    import torch
    from yolov3 import _hip
    lib = _hip.lib()
    assert _hip.capabilities() & _hip.CAP_LAUNCH_LOG == 2048
    assert lib.y3_debug_launch_log_end(None, 0, None) != 0 and b"no launch log" in lib.y3_last_error()
    assert lib.y3_debug_launch_log_begin() == 0
    assert lib.y3_debug_launch_log_begin() != 0 and b"already" in lib.y3_last_error()
    need = ctypes.c_size_t(99)
    assert lib.y3_debug_launch_log_end(None, 0, ctypes.byref(need)) != 0 and need.value == 1      # the size query: an empty log
    buf = ctypes.create_string_buffer(b"x" * 8, 8)
    assert lib.y3_debug_launch_log_end(buf, 8, None) == 0 and buf.value == b""
    assert lib.y3_debug_launch_log_end(buf, 8, None) != 0                                         # ended
    if torch.cuda.is_available():
        pytest.skip("fake device addresses must never reach a library that can see a GPU (the GPU tests take real logs)")
    with _hip.launch_log() as log:
        assert lib.y3_cxywh_to_tlbr(1 << 44, 1 << 45, 4, 4, None) != 0                            # no device: the launch fails
        assert lib.y3_cxywh_to_tlbr_float(1 << 44, 1 << 45, 4, 4, _hip.Y3_F64, None) != 0
    names = {k[".name"] for k in kernels}
    assert len(log.names) == 2 and log.symbols == sorted(set(log.names)) and set(log.names) <= names, log.names
    assert all("cxywh_to_tlbr_kernel" in n for n in log.names)
