"""CPU-side checks of the built library's device code (no GPU needed): the shared library carries gfx950 code objects
only, every kernel's register / LDS budget is inside the CU's limits and no kernel spills registers to scratch
memory.  Parses the clang offload bundles and the AMDGPU metadata notes of libyolov3_hip.so directly."""
import os
import struct

import msgpack
import pytest

from golden_util import ROOT

LIB = os.path.join(ROOT, "pytorch-yolov3_amd", "lib", "libyolov3_hip.so")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _code_objects(data):
    """(target triple, ELF bytes) of every device entry of every offload bundle in the file."""
    pos = 0
    while True:
        i = data.find(MAGIC, pos)
        if i < 0:
            return
        nent = struct.unpack_from("<Q", data, i + 24)[0]
        off = i + 32
        for _ in range(nent):
            o, sz, tl = struct.unpack_from("<QQQ", data, off)
            triple = data[off + 24:off + 24 + tl].decode()
            off += 24 + tl
            if sz and not triple.startswith("host"):
                yield triple, data[i + o:i + o + sz]
        pos = i + 24


def _kernels(elf):
    """amdhsa.kernels entries of one code object (NT_AMDGPU_METADATA note, msgpack)."""
    shoff = struct.unpack_from("<Q", elf, 0x28)[0]
    shentsize, shnum = struct.unpack_from("<HH", elf, 0x3A)
    for k in range(shnum):
        sh = elf[shoff + k * shentsize:shoff + (k + 1) * shentsize]
        if struct.unpack_from("<I", sh, 4)[0] != 7:          # SHT_NOTE
            continue
        so, ss = struct.unpack_from("<QQ", sh, 0x18)
        p = so
        while p < so + ss:
            namesz, descsz, ntype = struct.unpack_from("<III", elf, p)
            d0 = p + 12 + ((namesz + 3) & ~3)
            if ntype == 32 and elf[p + 12:p + 12 + namesz].startswith(b"AMDGPU"):
                md = msgpack.unpackb(elf[d0:d0 + descsz], raw=False, strict_map_key=False)
                for kern in md.get("amdhsa.kernels", []):
                    yield kern
            p = d0 + ((descsz + 3) & ~3)


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(LIB):
        pytest.skip("library not built (python -c 'import __graft_entry__ as g; g.build()')")
    data = open(LIB, "rb").read()
    objs = list(_code_objects(data))
    assert objs, "no device code in the library"
    out = []
    for triple, elf in objs:
        assert "gfx950" in triple, triple                    # one target, no multi-arch fallbacks
        out.extend(_kernels(elf))
    return out


def test_library_has_the_hot_path_kernels(kernels):
    names = " ".join(k[".name"] for k in kernels)
    for needle in ("conv_halo_ws_kernel", "conv_patch_wsp_kernel", "conv_igemm2_kernel", "conv_igemm3_kernel",
                   "conv_stem_s2_fused_kernel", "conv_resblock_fused_kernel", "yolo_decode_kernel", "detect_kernel",
                   "pack_records_kernel", "resize"):
        assert needle in names, needle


def test_no_kernel_spills_and_budgets_fit_a_cu(kernels):
    for k in kernels:
        name = k[".name"]
        assert k[".private_segment_fixed_size"] == 0, (name, "uses scratch memory (register spills)")
        assert k[".vgpr_count"] + k.get(".agpr_count", 0) <= 512, name
        assert k[".group_segment_fixed_size"] <= 160 * 1024, name
        assert k[".wavefront_size"] == 64, name


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


# ---- the census of compiled instances (tests/kernel_census.py) ---------------------------------------------------------------

def _census():
    import kernel_census as census
    if not os.path.exists(census.FIXTURE):
        pytest.fail("tests/golden/kernel_instances.json is missing (tools/make_kernel_instances.py writes it on an MI355X)")
    return census, census.load()


def test_every_compiled_kernel_is_launched_by_a_footprint_case_or_provably_by_nothing(kernels):
    """Coverage: every ``.name`` of the library's code objects is in the union of the fixture's ``footprint`` map -- a one-op
    test with the oracle gate, the strided / poisoned run and the byte-for-byte footprint check launched it on an MI355X --
    or in ``kernel_census.UNREACHABLE`` with the chooser condition that excludes it.  Never both: no recorded GPU test
    launches an UNREACHABLE symbol."""
    census, fixture = _census()
    library = {k[".name"] for k in kernels}
    t = census.totals(fixture, library)
    print("kernel census: %(symbols)d symbols, %(covered)d covered by footprint cases, %(unreachable)d unreachable" % t)
    rep = census.report(fixture, library)
    bad = [m for m in census.failures(fixture, library) if "footprint case" in m or "UNREACHABLE that" in m]
    assert not rep["uncovered"] and not rep["unreachable_but_launched"], "\n".join(bad)
    assert t["covered"] + t["unreachable"] == t["symbols"]
    for sym, reason in census.UNREACHABLE.items():
        assert ".hip:" in reason, "UNREACHABLE[%s] names no chooser line" % sym


def test_census_names_no_kernel_the_library_lacks(kernels):
    """Stale check: every symbol named in the fixture or in UNREACHABLE exists in the library (a removed or renamed instance
    must leave the record too)."""
    census, fixture = _census()
    library = {k[".name"] for k in kernels}
    assert not census.report(fixture, library)["stale"], "\n".join(m for m in census.failures(fixture, library) if "does not hold" in m)
    assert set(fixture) == {"footprint", "contention"} and fixture["footprint"] and fixture["contention"]
    for table in fixture.values():
        for key, syms in table.items():
            assert syms == sorted(set(syms)) and syms, key


def test_every_run_ahead_instance_runs_beside_the_copy_kernel(kernels):
    """Contention: every instance of the register-destination run-ahead families -- conv1x1_dw_kernel with both HEAD values,
    conv_dw48_kernel, conv_halo_dw_kernel: the kernels whose template parameter sets their wait counts -- is in the union of
    the fixture's ``contention`` map, or UNREACHABLE."""
    census, fixture = _census()
    library = {k[".name"] for k in kernels}
    t = census.totals(fixture, library)
    print("kernel census: %(run_ahead)d run-ahead instances, %(under_contention)d under contention" % t)
    assert t["run_ahead"] >= 2 * (9 + 5 + 14 + 3), t          # (both 16-bit types of the y3_ints lists as they stand)
    assert not census.report(fixture, library)["not_under_contention"], "\n".join(
        m for m in census.failures(fixture, library) if "contention case" in m)


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
