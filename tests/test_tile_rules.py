"""The rules of a tile launch on the exact engine (python-soxr_amd/csrc/tile_rules.h: kernel family, periods / slabs / blocks,
waves per workgroup, the planar kernels' slab size and unit split, the small and mid forms of the general-period kernel, the
splits and the XCD-aware ids, TileForm) on the CPU: tests/c/tile_rules_check.cpp states each slowly and independently over a
table of real geometries and over random ones, and compares — every period of a job in exactly one block and no block empty,
the kernels' own walks replayed over the chosen (waves, grid.z or xz, halves) so that every row tile or planar unit of a slab is
computed exactly once and every id of an XCD-mapped grid decodes once or idles, the waves rule against a recount, planes_form
against its cost formula, the LDS bytes of every form within 160 KiB and the halves form's scratch behind its slab, the family
truth table, a ragged launch of equal clips against the equal-length job.  It is a stand-alone program built with the host
compiler — once plain, once with the address and undefined-behaviour sanitizers — and run; nothing of it is loaded into
this process."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "python-soxr_amd", "csrc")

BUILDS = {
    "plain": ["-O1"],
    "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
}
RULES = ("tile_big", "tile_family", "tile_first_period", "tile_form", "tile_form_ragged", "tile_kind_name")
# (the rules tile_form and tile_form_ragged are made of; the launch layer calls the two and nothing beneath them)
PARTS = ("tile_periods", "tile_blocks", "tile_slabs", "tile_waves", "planes_form", "planes_slab", "general_slab16", "mfma64_pb", "units_per_slab", "v1_small", "v1_mid",
         "planar_split", "xcd_grid", "row_tile_split", "row_split", "halves_form")
KERNELS = ("k_tile<", "k_tile_mfma<", "k_tile_mfma_p<", "k_tile_mfma64_p<")


def _host_compiler():
    for name in (os.environ.get("CXX"), "g++", "c++", "clang++", "/opt/rocm/lib/llvm/bin/clang++"):
        if name and shutil.which(name):
            return shutil.which(name)
    raise AssertionError("no host C++ compiler found (g++, c++ or clang++)")


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def test_header_needs_no_hip():
    """The rules compile and run on a CPU alone: the header includes the standard library, nothing of HIP or the engine, and
    reads no switch but through its arguments."""
    text = _read("tile_rules.h")
    includes = [line.split()[1] for line in text.splitlines() if line.startswith("#include")]
    assert "<cstdint>" in includes
    assert not [i for i in includes if "hip" in i.lower() or i.startswith('"')], includes
    assert "__global__" not in text and "__device__" not in text
    assert not re.search(r"switches\(\)\.", text)


def test_the_launcher_uses_the_header():
    """kernels.hip decides through the header's functions, not through copies: every rule is called — the two forms are made of
    every part — and none of the constants the header owns is written out in the launch layer; one geometry type."""
    src, rules = _read("kernels.hip"), _read("tile_rules.h")
    assert '#include "tile_rules.h"' in src
    host = src[src.index("static TileSwitches tile_switches()"):src.index("bool resident_post(")]  # the launch layer: behind the kernels
    assert "__global__" not in host
    for name in RULES:
        assert name + "(" in host, name
    forms = rules[rules.index("inline TileForm tile_form("):]
    for name in PARTS:
        assert name + "(" in forms, name
    for copy in (r"2048", r"6\s*\*\s*256", r"0\.276", r"0\.82", r"0\.53", r"2\s*\*\s*3\s*\*\s*256", r"best_waste", r"waste\s*<", r"\b4096\b", r"16\s*\*\s*g\w*\.Lc",
                 r"\+\s*7\)\s*/\s*8", r"/\s*g\w*\.Lc\s*-"):
        assert not re.search(copy, host), "kernels.hip's launch layer restates a rule of tile_rules.h: " + copy
    assert len(re.findall(r"\bstruct TileGeom\b", src + rules)) == 1 and "struct TileGeom {" in rules
    # switches() reaches the rules in one place
    assert host.count("tile_switches()") == 3 and src.count("TileSwitches s;") == 1


def test_tile_kernel_instances_are_named_in_one_function():
    src = _read("kernels.hip")
    host = src[src.index("static TileSwitches tile_switches()"):src.index("bool resident_post(")]
    a = host.index("static void (*tile_kernel(")
    b = host.index("\n}\n", a)
    for k in KERNELS:
        assert k in host[a:b], k
        assert k not in host[:a] and k not in host[b:], "a tile kernel instance named outside tile_kernel: " + k
    assert host.index("tile_args(") < a < host.index("tile_trace_begin") < host.index("static const char *launch_tile(")


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_rules_against_slow_statements(build, tmp_path):
    exe = str(tmp_path / ("tile_rules_check_" + build))
    cxx, flags = _host_compiler(), list(BUILDS[build])
    if build == "sanitized" and "clang" not in os.path.basename(cxx):
        flags += ["-static-libasan", "-static-libubsan"]  # the runtimes inside the program, as clang links them anyway
    cmd = [cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, os.path.join(ROOT, "tests", "c", "tile_rules_check.cpp"), "-o", exe]
    made = subprocess.run(cmd, capture_output=True, text=True)
    assert made.returncode == 0, made.stdout + made.stderr
    ran = subprocess.run([exe], capture_output=True, text=True)
    print(ran.stdout[-3000:])
    assert ran.returncode == 0, ran.stdout[-3000:] + ran.stderr[-3000:]
    assert re.search(r"\b[1-9]\d* checks, 0 failed", ran.stdout)
