"""The census of compiled kernel instances: which device function every value-checked one-op test launches.

The library is compiled by INSTANCE: below the name ``y3_plan_op_kernel`` reports, the ``y3_ints<...>`` lists of the .hip files
expand a family into separately compiled device functions, each with its own unroll, LDS image and (in the direct-weights
kernels) hand-counted waits.  ``tests/golden/kernel_instances.json`` records, from an MI355X run of tools/make_kernel_instances.py,
the code-object symbols (the ``.name`` of the AMDGPU metadata, mangled) that every case of tests/test_gpu_footprint.py and
tests/test_gpu_contention.py launches, taken with the library's launch log (``y3_debug_launch_log_begin`` / ``_end``).  The rules
below hold that record against the kernels the built library holds; tests/test_code_object.py runs them without a GPU, the tool
runs them before it writes, and the GPU tests assert that they launch exactly what is recorded."""
import json
import os
import subprocess

from golden_util import ROOT

FIXTURE = os.path.join(ROOT, "tests", "golden", "kernel_instances.json")
CXXFILT = "/opt/rocm/llvm/bin/llvm-cxxfilt"

# The register-destination run-ahead families (tests/test_gpu_contention.py): the kernels whose template parameter sets the
# counts of their hand-counted waits.  Selected by the template's identifier inside the mangled name.
RUN_AHEAD = ("conv1x1_dw_kernel", "conv_dw48_kernel", "conv_halo_dw_kernel")

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


def load():
    with open(FIXTURE) as f:
        return json.load(f)


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


def report(fixture, library):
    """The three rules on ``fixture`` ({"footprint": {key: [symbols]}, "contention": {...}}) and ``library`` (the ``.name`` of
    every kernel of the built library): {rule: sorted offending symbols}, all empty when the census is whole."""
    library = set(library)
    foot, cont = union(fixture["footprint"]), union(fixture["contention"])
    unreachable = set(UNREACHABLE)
    run_ahead = {s for s in library if any(of_family(s, f) for f in RUN_AHEAD)}
    return {
        # coverage: every kernel is launched by a footprint case, or provably by nothing -- never both
        "uncovered": sorted(library - foot - unreachable),
        "unreachable_but_launched": sorted(unreachable & (foot | cont)),
        # stale: every recorded or excluded symbol exists
        "stale": sorted((foot | cont | unreachable) - library),
        # contention: every run-ahead instance runs beside the copy kernel
        "not_under_contention": sorted(run_ahead - cont - unreachable),
    }


def failures(fixture, library):
    """[message per broken rule], symbols demangled where the tool exists"""
    rep = report(fixture, library)
    names = demangle([s for v in rep.values() for s in v])
    what = {"uncovered": "kernels no footprint case launches and UNREACHABLE does not hold",
            "unreachable_but_launched": "kernels listed as UNREACHABLE that a recorded GPU test launches",
            "stale": "symbols of the fixture or of UNREACHABLE that the library does not hold",
            "not_under_contention": "run-ahead instances no contention case launches"}
    return ["%d %s:\n  %s" % (len(v), what[k], "\n  ".join(names[s] for s in v)) for k, v in rep.items() if v]


def totals(fixture, library):
    library = set(library)
    return {"symbols": len(library), "covered": len(library & union(fixture["footprint"])),
            "unreachable": len(library & set(UNREACHABLE)),
            "run_ahead": sum(1 for s in library if any(of_family(s, f) for f in RUN_AHEAD)),
            "under_contention": len({s for s in library & union(fixture["contention"]) if any(of_family(s, f) for f in RUN_AHEAD)})}
