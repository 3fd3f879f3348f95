"""Builds the reference's two kernels (d_render, d_basicDataProcessing) for the CPU.

TEST INFRASTRUCTURE ONLY.  The reference's kernel file is read from the directory
named by VR_REFERENCE_DIR (default: the mount named in BASELINE.md), cut before
its flexible-block prepass, edited by matched text, written to oracle/_ref/gen/
and compiled with the shim headers of oracle/ref/shim/ and oracle/ref/ref_driver.cpp
into one shared library per variant under oracle/_ref/.  Nothing under
oracle/_ref/ is committed.  Where the reference directory does not exist this
does nothing and deletes nothing: libraries built earlier stay usable.

Every pattern must match an exact number of times, else the build stops: a
reference whose text has moved is to be looked at, not guessed at.
"""
from __future__ import annotations

import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(os.path.dirname(HERE), "_ref")
GEN = os.path.join(OUT, "gen")
ENV = "VR_REFERENCE_DIR"
DEFAULT_DIR = "/root/reference"
KERNEL_FILE = "volumeRender_kernel.cu"

# -Bsymbolic: several variants live in one process, each bound to its own globals;
# -w: the reference's text is compiled as it is, its warnings are not ours to fix
BASE_FLAGS = ["-std=c++17", "-O2", "-fno-fast-math", "-fPIC", "-shared", "-fopenmp", "-w",
              "-Wl,-Bsymbolic"]
CANONICAL = ["-ffp-contract=off"]
CONTRACTED = ["-ffp-contract=fast", "-mfma"]

# the text ends where the flexible-block prepass begins (its kernels use shared
# memory, barriers and float atomics: out of scope)
CUT = "__device__ int4 corner[32768];"
GUARD = "#ifndef _VOLUMERENDER_KERNEL_CU_"
# (pattern, replacement, expected matches); {nbins} is the variant's bin count
EDITS = [
    # fractalDecoding / flexibleFractalDecoding return the address of a local;
    # the oracle's reading is "the result is the decoded array" (vr_oracle.c)
    ("\tfloat decoded[nBins];", "\tstatic thread_local float decoded[nBins];", 1),
    ("\tfloat decoded[flexNBin];", "\tstatic thread_local float decoded[flexNBin];", 1),
    ("const int nBins = 32;", "const int nBins = {nbins};", 1),
]
# wrong on purpose, for the canary of tests/test_reference_text.py: the far exit
# taken one step early.  (Swapping the far exit with the opacity exit alone
# cannot change a pixel: both leave the loop after the same composite.)
EXIT_CANARY = [("if (t > tfar)", "if (t + tstep > tfar)", 1)]

# name -> (bins, extra edits, flags)
VARIANTS = {
    "b32": (32, [], CANONICAL),
    "b8": (8, [], CANONICAL),
    "b32_fma": (32, [], CONTRACTED),
    "b32_exit_canary": (32, EXIT_CANARY, CANONICAL),
}


class RecipeError(RuntimeError):
    pass


def reference_dir() -> str:
    return os.environ.get(ENV, DEFAULT_DIR)


def reference_present() -> bool:
    """the reference's directory is there and its kernel file can be read"""
    return os.access(os.path.join(reference_dir(), KERNEL_FILE), os.R_OK)


def lib_path(name: str) -> str:
    return os.path.join(OUT, f"libref_{name}.so")


def _count(text: str, pat: str, want: int, where: str) -> None:
    n = text.count(pat)
    if n != want:
        raise RecipeError(f"{where}: expected {want} match(es) of {pat!r}, found {n}; the "
                          "reference's text is not the one this recipe was written for")


def generate(src: str, nbins: int, extra) -> str:
    _count(src, CUT, 1, "cut point")
    cut = src.index(CUT)
    text = src[:src.rfind("\n", 0, cut) + 1]
    _count(text, GUARD, 1, "include guard")
    _count(text, "#endif", 0, "include guard")
    for pat, rep, want in EDITS + list(extra):
        _count(text, pat, want, "edit")
        text = text.replace(pat, rep.format(nbins=nbins))
    return text + "\n#endif\n"


def _inputs():
    shim = os.path.join(HERE, "shim")
    return ([os.path.join(HERE, "ref_driver.cpp"), os.path.abspath(__file__)] +
            [os.path.join(shim, f) for f in sorted(os.listdir(shim))])


def build(force: bool = False, verbose: bool = False) -> list:
    """Build every variant that is missing or older than its inputs; returns the
    library paths, [] where there is no reference directory."""
    ref = reference_dir()
    kernel = os.path.join(ref, KERNEL_FILE)
    if not reference_present():
        if verbose:
            print(f"build_ref: no readable {KERNEL_FILE} under {ref}; nothing to do")
        return []
    with open(kernel, encoding="utf-8", errors="replace") as f:
        src = f.read()
    os.makedirs(GEN, exist_ok=True)
    newest = max(os.path.getmtime(p) for p in _inputs() + [kernel])
    cxx = os.environ.get("CXX", "g++")
    libs = []
    for name, (nbins, extra, flags) in VARIANTS.items():
        so = lib_path(name)
        libs.append(so)
        if not force and os.path.exists(so) and os.path.getmtime(so) >= newest:
            continue
        gen = os.path.join(GEN, f"kernel_{name}.inc")
        with open(gen, "w", encoding="utf-8") as f:
            f.write(generate(src, nbins, extra))
        tmp = so + ".tmp"
        cmd = [cxx] + BASE_FLAGS + flags + [
            "-I", os.path.join(HERE, "shim"), f'-DVR_REF_KERNEL_TEXT="{gen}"',
            os.path.join(HERE, "ref_driver.cpp"), "-o", tmp]
        if verbose:
            print(" ".join(cmd))
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RecipeError(f"compiling the reference variant {name} failed:\n{r.stderr[-4000:]}")
        os.replace(tmp, so)
    return libs


def selfcheck() -> None:
    """The driver's stand-alone program (its own main) built with the host
    sanitizers and run once per bin count.  Never for code loaded into Python."""
    if not build():
        print("build_ref: no reference directory; nothing to check")
        return
    for name in ("b32", "b8"):
        exe = os.path.join(OUT, f"selfcheck_{name}")
        flags = [f for f in BASE_FLAGS if f not in ("-shared", "-Wl,-Bsymbolic")]
        cmd = [os.environ.get("CXX", "g++")] + flags + CANONICAL + [
            "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
            "-DVR_REF_SELFCHECK_MAIN", "-I", os.path.join(HERE, "shim"),
            f'-DVR_REF_KERNEL_TEXT="{os.path.join(GEN, f"kernel_{name}.inc")}"',
            os.path.join(HERE, "ref_driver.cpp"), "-o", exe]
        subprocess.run(cmd, check=True)
        subprocess.run([exe], check=True)


if __name__ == "__main__":
    if "--selfcheck" in sys.argv:
        selfcheck()
        sys.exit(0)
    try:
        for p in build(force="--force" in sys.argv, verbose=True):
            print(p)
    except RecipeError as e:
        sys.exit(f"build_ref: {e}")
