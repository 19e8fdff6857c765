"""The census of compiled kernel instances: which device function every value-checked one-op test launches.

The libraries are compiled by INSTANCE: below the name ``y3_plan_op_kernel`` reports, the ``y3_ints<...>`` lists of the .hip files
expand a family into separately compiled device functions, each with its own unroll, LDS image and (in the direct-weights
kernels) hand-counted waits.  Per library of ``LIBRARIES`` a fixture under tests/golden records, from an MI355X run of
tools/make_kernel_instances.py, the code-object symbols (the ``.name`` of the AMDGPU metadata, mangled) that every case of its
footprint and contention tests launches, taken with the library's launch log (``y3_debug_launch_log_begin`` / ``_end``).  The rules
of ``report`` hold that record against the kernels the built library holds; tests/test_code_object.py runs them without a GPU,
the tool runs them before it writes, and the GPU tests assert through ``assert_census`` that they launch exactly what is recorded."""
import collections
import contextlib
import json
import os
import subprocess

import code_object
from golden_util import GOLDEN

CXXFILT = "/opt/rocm/llvm/bin/llvm-cxxfilt"

# The register-destination run-ahead families (tests/test_gpu_contention.py): the kernels whose template parameter sets the
# counts of their hand-counted waits.  Selected by the template's identifier inside the mangled name.
RUN_AHEAD = ("conv1x1_dw_kernel", "conv_dw48_kernel", "conv_halo_dw_kernel")
EVERY_KERNEL = "*"          # in place of a list of families: every kernel of the library is a run-ahead kernel

# Instances no y3_op can reach under any y3_options: {symbol: the chooser condition that excludes it}.  They stay compiled
# (removing one moves the device code); a later change may delete them from their y3_ints list.
_HALO_WS_33 = ("conv_halo.hip:1221-1225 (halo_strip_geom, the one place that sizes the ring) takes three weight slots only when four "
               "do not fit: na > 12 or 4 * 16 KiB + 2 * na * 4 KiB > 160 KiB, i.e. na >= 13.  At 192-pixel tiles (MI = 3) na = "
               "ceil((196 + 2 W) / 32) (:1210-1211), and conv_halo.hip:1271 (y3_conv_halo_ws_fits, required by y3_choose_conv_halo "
               ":1366) asks the same function about 256-pixel tiles and so admits only ceil((260 + 2 W) / 32) <= 14, i.e. W <= 94, "
               "where the 192-pixel tile has na <= 12: the loop always stops at four slots, which the chooser records (:1369-1373)")
UNREACHABLE = {
    "_ZN12_GLOBAL__N_119conv_halo_ws_kernelIfLi3ELi3EEEvNS_8HaloArgsE": _HALO_WS_33,
    "_ZN12_GLOBAL__N_119conv_halo_ws_kernelIDF16bLi3ELi3EEEvNS_8HaloArgsE": _HALO_WS_33,
    "_ZN12_GLOBAL__N_119conv_halo_ws_kernelIDF16_Li3ELi3EEEvNS_8HaloArgsE": _HALO_WS_33,
}

# One record per shared library: its file under pytorch-yolov3_amd/lib, its fixture under tests/golden (None: the tile-merge
# library is one kernel, no census), its run-ahead families and its unreachable symbols.  A new kernel family in a library of
# its own is one more row here and one more list of tests in tools/make_kernel_instances.py.
Library = collections.namedtuple("Library", "file fixture run_ahead unreachable")
LIBRARIES = {
    "main": Library("libyolov3_hip.so", "kernel_instances.json", RUN_AHEAD, UNREACHABLE),
    "grouped": Library("libyolov3_hip_grouped.so", "kernel_instances_grouped.json", (), {}),
    "block": Library("libyolov3_hip_block.so", "kernel_instances_block.json", EVERY_KERNEL, {}),
    "attn": Library("libyolov3_hip_attn.so", "kernel_instances_attn.json", (), {}),
    "tilemerge": Library("libyolov3_hip_tilemerge.so", None, (), {}),
}


def fixture_path(name="main"):
    return os.path.join(GOLDEN, LIBRARIES[name].fixture)


def load(name="main"):
    with open(fixture_path(name)) as f:
        return json.load(f)


def kernels(name="main"):
    """the amdhsa.kernels entries of the built library ``name`` (tests/code_object.py: gfx950 device code only)"""
    return code_object.library_kernels(LIBRARIES[name].file)


def symbols(name="main"):
    return {k[".name"] for k in kernels(name)}


def of_family(symbol, identifier):
    """whether ``symbol`` is an instance of the template ``identifier`` (its length-prefixed form in the mangled name)"""
    return "%d%sI" % (len(identifier), identifier) in symbol


def demangle(symbols):
    """{symbol: readable name}; the symbol itself where llvm-cxxfilt is not installed"""
    symbols = list(symbols)
    if symbols and os.path.exists(CXXFILT):
        out = subprocess.run([CXXFILT], input="\n".join(symbols) + "\n", capture_output=True, text=True).stdout.split("\n")
        if len(out) >= len(symbols):
            return dict(zip(symbols, out))
    return {s: s for s in symbols}


def union(table):
    return set().union(*table.values()) if table else set()


def _sets(name, fixture, library):
    """(library, footprint union, contention union, unreachable, run-ahead instances); a fixture without a ``contention`` table
    (the attention library's) reads as one with an empty table"""
    lib, library = LIBRARIES[name], set(library)
    run_ahead = library if lib.run_ahead == EVERY_KERNEL else {s for s in library if any(of_family(s, f) for f in lib.run_ahead)}
    return library, union(fixture["footprint"]), union(fixture.get("contention")), set(lib.unreachable), run_ahead


def report(name, fixture, library):
    """The four rules of library ``name`` on ``fixture`` ({"footprint": {key: [symbols]}, "contention": {...}}) and ``library``
    (the ``.name`` of every kernel of the built library): {rule: sorted offending symbols}, all empty when the census is whole.

    Where nothing is unreachable the second rule cannot fire and the first is "every kernel is launched by a footprint case".
    With every kernel run-ahead (block) the fourth is "every kernel is launched by a contention case": uncovered, stale and
    quiet-only, the three lists the block library's own report gave.  With no run-ahead family and an empty or absent contention
    table (grouped, attn) the fourth cannot fire either, and what is left is the two rules those libraries' reports held."""
    library, foot, cont, unreachable, run_ahead = _sets(name, fixture, library)
    return {
        # coverage: every kernel is launched by a footprint case, or provably by nothing -- never both
        "uncovered": sorted(library - foot - unreachable),
        "unreachable_but_launched": sorted(unreachable & (foot | cont)),
        # stale: every recorded or excluded symbol exists
        "stale": sorted((foot | cont | unreachable) - library),
        # contention: every run-ahead instance runs beside the copy kernel
        "not_under_contention": sorted(run_ahead - cont - unreachable),
    }


WHAT = {"uncovered": "kernels no footprint case launches and UNREACHABLE does not hold",
        "unreachable_but_launched": "kernels listed as UNREACHABLE that a recorded GPU test launches",
        "stale": "symbols of the fixture or of UNREACHABLE that the library does not hold",
        "not_under_contention": "run-ahead instances no contention case launches"}


def failures(name, fixture, library):
    """[message per broken rule], symbols demangled where the tool exists"""
    rep = report(name, fixture, library)
    names = demangle([s for v in rep.values() for s in v])
    return ["%s: %d %s:\n  %s" % (name, len(v), WHAT[k], "\n  ".join(names[s] for s in v)) for k, v in rep.items() if v]


def totals(name, fixture, library):
    library, foot, cont, unreachable, run_ahead = _sets(name, fixture, library)
    return {"symbols": len(library), "covered": len(library & foot), "unreachable": len(library & unreachable),
            "run_ahead": len(run_ahead), "under_contention": len(run_ahead & cont)}


def summary(name, fixture, library):
    return ("%(symbols)d symbols, %(covered)d covered by footprint cases, %(unreachable)d unreachable; %(run_ahead)d run-ahead "
            "instances, %(under_contention)d under contention" % totals(name, fixture, library))


# ------------------------------------------------------------------------------------------------ the launch log of the GPU tests

LAUNCHED = []           # the sorted symbol set of every logged call since a test (or the census tool) last cleared it
FRAGMENT_LAUNCHED = []  # ... and of every y3_conv_make_fragment_weights call inside test_gpu_footprint._run
FRAGMENT_KEY = "y3_conv_make_fragment_weights"          # (a kernel of the main library, whichever library's op the copy is for)
_recording = None          # inside ``recording()``: {library: {table: {key: symbols}}}


def logged(call):
    """``call()`` under the library's launch log; what it launched is appended to LAUNCHED"""
    from yolov3 import _hip as H
    with H.launch_log() as log:
        out = call()
    LAUNCHED.append(log.symbols)
    return out


@contextlib.contextmanager
def recording():
    """While open, ``assert_census`` records what was launched into the dict this yields, {library: {table: {key: symbols}}},
    instead of comparing it with the fixtures: tools/make_kernel_instances.py runs the GPU tests inside it."""
    global _recording
    assert _recording is None, "census.recording() is already open"
    _recording = record = {}
    try:
        yield record
    finally:
        _recording = None


def is_recording():
    return _recording is not None


def assert_census(key, table="footprint", library="main", launched=None):
    """Every symbol set of ``launched`` -- by default every logged call since the last clear: LAUNCHED, which this clears -- is
    exactly what the fixture of ``library`` records for ``key`` in ``table``."""
    if launched is None:
        launched = LAUNCHED[:]
        del LAUNCHED[:]
    assert launched, key
    if _recording is not None:
        assert all(got == launched[0] for got in launched), (key, launched)
        assert _recording.setdefault(library, {}).setdefault(table, {}).setdefault(key, launched[0]) == launched[0], key
        return
    want = load(library).get(table, {}).get(key)
    assert want is not None, "tests/golden/%s has no %s entry %r: run tools/make_kernel_instances.py --library %s" % (
        LIBRARIES[library].fixture, table, key, library)
    names = demangle(set(want).union(*launched))
    for got in launched:
        assert got == want, "%s launched\n  %s\nrecorded\n  %s" % (key, "\n  ".join(names[s] for s in got),
                                                                 "\n  ".join(names[s] for s in want))
