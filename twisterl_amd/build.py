"""Builds the HIP collector library for gfx950 with hipcc (in-tree, no JIT cache).

    python -m twisterl_amd.build            # incremental
    python -m twisterl_amd.build --force

Output: twisterl_amd/lib/libtwisterl_hip.so (git-ignored; it travels to the GPU box with the tree).
hipcc cross-compiles without a GPU, so this also runs in the CPU-only build container.
"""
from __future__ import annotations

import glob
import os
import shutil
import subprocess
import sys

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
# The diagnostic variant (TW_ABLATE=1 in the environment: -DTW_ABLATE, cycle stamps) is a DIFFERENT
# library in its own directory: the product library is never overwritten by an instrumented build, and a process loads the
# instrumented one only while TW_ABLATE is set.
ABLATE = bool(os.environ.get("TW_ABLATE"))
# A measurement variant (TW_VARIANT=<name> with TW_EXTRA_FLAGS=-D..., the two sides of an A/B experiment) likewise
# builds into, and loads from, a directory of its own.
VARIANT = os.environ.get("TW_VARIANT", "")
LIB_DIR = os.path.join(PKG, "lib", "ablate") if ABLATE else os.path.join(PKG, "lib", "variants", VARIANT) if VARIANT else os.path.join(PKG, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libtwisterl_hip_ablate.so" if ABLATE else f"libtwisterl_hip_{VARIANT}.so" if VARIANT else "libtwisterl_hip.so")
SOURCES = sorted(os.path.basename(p) for p in glob.glob(os.path.join(CSRC, "*.hip")))
# every header is a dependency of every object (an edited header must never leave a stale object behind)
HEADERS = sorted(glob.glob(os.path.join(CSRC, "*.hpp"))) + sorted(glob.glob(os.path.join(ROOT, "include", "*.h")))

# -ffp-contract=off: the numeric spec allows only the explicit fma() calls
# -pragma-unroll-threshold: the pinned MFMA schedules are fully unrolled position loops whose bodies call constexpr
# schedule functions; the default limit (16K IR instructions before folding) would leave them as real loops
FLAGS = ["-O3", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-slp-vectorize", "-std=c++17", "-fPIC",
         "-mllvm", "-pragma-unroll-threshold=400000",
         "-fno-gpu-rdc", "-Wall", "-Wno-unused-function"]


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found (looked at $HIPCC, PATH, /opt/rocm/bin/hipcc)")


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


ASM_DIR = os.path.join(LIB_DIR, "asm")          # the device assembly of every object (what scripts/scan_mfma_hazards.py reads)
_TEMP_SUFFIXES = (".bc", ".hipi", ".out", ".out.resolution.txt", ".hipfb", "-host-x86_64-unknown-linux-gnu.s", "-hip-amdgcn-amd-amdhsa-gfx950.o")


def _keep_device_asm(stem: str) -> None:
    """-save-temps=obj leaves every intermediate file beside the object: the gfx950 assembly (the text the object was assembled
    from) moves to lib/asm/, the rest goes."""
    os.makedirs(ASM_DIR, exist_ok=True)
    for f in os.listdir(LIB_DIR):
        if not f.startswith(stem + "-") and not f.startswith(stem + ".hip-"):
            continue
        path = os.path.join(LIB_DIR, f)
        if f == stem + "-hip-amdgcn-amd-amdhsa-gfx950.s":
            os.replace(path, os.path.join(ASM_DIR, stem + ".s"))
        elif f.endswith(_TEMP_SUFFIXES):
            os.remove(path)


def scan_hazards(verbose: bool = False) -> int:
    """MFMA wait-state check of the assembly the library was built from (scripts/scan_mfma_hazards.py): inline-asm MFMAs get no
    padding from hipcc, so a hazard there is a BUILD ERROR, not something a parity test may or may not catch."""
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import scan_mfma_hazards as scan
    finally:
        sys.path.pop(0)
    files = sorted(glob.glob(os.path.join(ASM_DIR, "*.s")))
    missing = [s for s in SOURCES if not os.path.exists(os.path.join(ASM_DIR, s.replace(".hip", ".s")))]
    if missing:
        raise RuntimeError(f"no device assembly for {missing}: rebuild with --force")
    report, mfmas = [], 0
    for f in files:
        hits, counts = scan.scan_file(f)
        mfmas += sum(counts.values())
        report += [f"{os.path.basename(f)}: {h}" for h in hits]
    if report:
        raise RuntimeError("MFMA hazards in the compiled kernels (scripts/scan_mfma_hazards.py):\n" + "\n".join(report[:40]))
    if verbose:
        print(f"[build] MFMA hazard scan: 0 in {mfmas} MFMAs of {len(files)} files")
    return mfmas


def build_library(force: bool = False, verbose: bool = False) -> str:
    os.makedirs(LIB_DIR, exist_ok=True)
    flags = list(FLAGS)
    if ABLATE:                           # the same kernels with cycle stamps (tw_common.hpp; TW_STAMPS=1 prints them)
        flags.append("-DTW_ABLATE")
    if os.environ.get("TW_EXTRA_FLAGS"):
        flags += os.environ["TW_EXTRA_FLAGS"].split()
    objs = []
    srcs = [s for s in SOURCES if os.path.exists(os.path.join(CSRC, s))]
    procs = []
    for s in srcs:
        src = os.path.join(CSRC, s)
        obj = os.path.join(LIB_DIR, s.replace(".hip", ".o"))
        objs.append(obj)
        if force or _stale(obj, [src] + HEADERS):
            cmd = [hipcc(), *flags, "-save-temps=obj", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-c", src, "-o", obj]
            if verbose:
                print(" ".join(cmd), flush=True)
            procs.append((s, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    for name, p in procs:
        out, _ = p.communicate()
        if p.returncode != 0:
            raise RuntimeError(f"hipcc failed on {name}:\n{out}")
        if verbose and out.strip():
            print(out)
        _keep_device_asm(name.replace(".hip", ""))
    # The scan belongs to the compile: whenever an object was rebuilt, all of the library's assembly is checked.  (A tree that
    # holds objects without their assembly -- the snapshot on the GPU box leaves lib/asm/ behind, .gpurunignore -- is not
    # recompiled for it; tests/test_mfma_hazards.py insists on the assembly where the library is built.)
    if procs:
        scan_hazards(verbose)
    if force or procs or _stale(LIB_PATH, objs):
        cmd = [hipcc(), "-shared", "-fPIC", "--offload-arch=gfx950", "-o", LIB_PATH, *objs]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"link failed:\n{r.stdout}")
    return LIB_PATH


DEVICE_ENV_DIR = os.path.join(LIB_DIR, "device_envs")     # (git-ignored with the rest of lib/)


def _scan_asm(paths, who: str) -> int:
    sys.path.insert(0, os.path.join(ROOT, "scripts"))
    try:
        import scan_mfma_hazards as scan
    finally:
        sys.path.pop(0)
    report, mfmas = [], 0
    for f in paths:
        hits, counts = scan.scan_file(f)
        mfmas += sum(counts.values())
        report += [f"{os.path.basename(f)}: {h}" for h in hits]
    if report:
        raise RuntimeError(f"MFMA hazards in {who} (scripts/scan_mfma_hazards.py):\n" + "\n".join(report[:40]))
    return mfmas


def build_device_env(header: str, type_name: str, name: str, out_dir: str = None, force: bool = False, search: bool = False,
                     wide: bool = False, wide_search: bool = False, fp16: bool = False, fp16_solve: bool = False,
                     fp16_search: bool = False, fp16x2: bool = False, fp16x2_solve: bool = False, basic: bool = False) -> str:
    """Compiles a user-written device environment (include/twisterl_device_env.hpp) into a loadable module:
    `#include "<header>"` + `TW_DEVICE_ENV(<type_name>, <name>)` with the library's own FLAGS (-ffp-contract=off: bit parity with the
    host path), the device assembly kept beside the module (<out_dir>/libtw_env_<name>.s) and scanned for MFMA hazards like the
    library's -- a hazard is a build error.  Returns the path of libtw_env_<name>.so (exports tw_device_env_<name>); rebuilt when the
    header or a library header is newer.  search=True emits `TW_DEVICE_ENV_SEARCH(...)` instead: the module then also holds the
    search kernel (twisterl_amd/csrc/tw_mcts_env.hpp), and AZCollector.collect and evaluate with MCTS run on the device; the struct
    may then have at most 128 bytes.  wide=True puts `#define TW_DEVICE_ENV_WIDE` in front of the header: NUM_ACTIONS may then be 1..31
    (the default build keeps 1..4); the generated source differs, so a module built one way is never taken from the cache as the other.  wide_search=True emits the define
    and `TW_DEVICE_ENV_WIDE_SEARCH(...)`: the search kernel for 1..31 actions (self-play and MCTS-guided evaluate of a wide environment
    on the device), the struct again at most 128 bytes; wide=True with search=True stays what it was, refused above four actions.
    fp16=True puts `#define TW_DEVICE_ENV_FP16` in front of the header, with any of the forms above: the module then also holds
    rollout_env16_kernel and the kernel that packs its binary16 weight image (twisterl_amd/csrc/tw_engine_generic16.hpp), and
    PPOCollector(precision="fp16").collect runs on the device; again the generated source differs, so the cache never serves one kind
    as the other.  fp16_solve=True implies fp16=True and puts `#define TW_DEVICE_ENV_FP16_SOLVE` in front of the header as well: the module
    then also holds solve_env16_kernel, and collector.evaluate / collector.solve with precision="fp16" (no MCTS) run on the device
    (DeviceEnv.fp16_solve says so); a third kind to the cache, for the same reason.  fp16_search=True implies fp16=True too, needs
    search=True or wide_search=True (ValueError otherwise, before anything is compiled) and puts `#define TW_DEVICE_ENV_FP16_SEARCH` in
    front of the header: the module then also holds mcts_env16_kernel, and AZCollector(precision="fp16").collect and
    collector.evaluate / collector.solve with MCTS and precision="fp16" run on the device (DeviceEnv.fp16_search says so); one more kind
    to the cache.  fp16x2=True implies fp16=True as well and puts `#define TW_DEVICE_ENV_FP16X2` in front of the header, with any of the
    forms and flags above: the module then also holds rollout_env16x2_kernel and the kernel that packs its two-plane binary16 weight
    image (twisterl_amd/csrc/tw_engine_generic16x2.hpp), and PPOCollector(precision="fp16x2").collect runs on the device
    (DeviceEnv.fp16x2 says so); one more kind to the cache.  fp16x2_solve=True implies fp16x2=True (and so fp16=True) and puts
    `#define TW_DEVICE_ENV_FP16X2_SOLVE` in front of the header as well, with any of the forms and flags above: the module then also holds
    solve_env16x2_kernel (twisterl_amd/csrc/tw_solve_env16x2.hpp), and collector.evaluate / collector.solve with precision="fp16x2" (no
    MCTS) run on the device (DeviceEnv.fp16x2_solve says so); one more kind to the cache.  basic=True puts `#define TW_DEVICE_ENV_BASIC` in front of the header, with any of the forms and flags
    above: the module then also holds pack_basic_view_kernel (twisterl_amd/csrc/tw_env_basic_view.hpp), and the f32 kernels the module
    has -- PPO collect, evaluate and solve, with a search form self-play and the MCTS-guided calls -- also run under the reference's
    DEFAULT policy, one common layer of 32 / 64 / 128 / 256 units and obs_size <= 256, which otherwise runs host-stepped (DeviceEnv.basic
    says so; fp16 / fp16x2 under such a policy stay "f32 only"); one more kind to the cache.  Every other combination of flags generates
    the source it generated before."""
    if fp16_search and not (search or wide_search):
        raise ValueError("build_device_env: fp16_search=True needs the search kernel: search=True or wide_search=True")
    fp16x2 = fp16x2 or fp16x2_solve
    fp16 = fp16 or fp16_solve or fp16_search or fp16x2
    if wide_search and search:
        raise ValueError("build_device_env: wide_search=True is a form of its own, not an addition to search=True")
    if not name.isidentifier() or not all(p.isidentifier() for p in type_name.split("::") if p) or not type_name.strip(":"):
        raise ValueError(f"build_device_env: name {name!r} / type {type_name!r} must be C identifiers (a template: give it an alias)")
    header = os.path.abspath(header)
    if not os.path.exists(header):
        raise FileNotFoundError(header)
    out_dir = os.path.abspath(out_dir or DEVICE_ENV_DIR)
    os.makedirs(out_dir, exist_ok=True)
    stem = f"libtw_env_{name}"
    so, asm, src = (os.path.join(out_dir, stem + ext) for ext in (".so", ".s", ".hip"))
    text = (f'// generated by twisterl_amd.build.build_device_env\n{"#define TW_DEVICE_ENV_WIDE" + chr(10) if wide or wide_search else ""}'
            f'{"#define TW_DEVICE_ENV_FP16" + chr(10) if fp16 else ""}{"#define TW_DEVICE_ENV_FP16_SOLVE" + chr(10) if fp16_solve else ""}{"#define TW_DEVICE_ENV_FP16_SEARCH" + chr(10) if fp16_search else ""}{"#define TW_DEVICE_ENV_FP16X2" + chr(10) if fp16x2 else ""}{"#define TW_DEVICE_ENV_FP16X2_SOLVE" + chr(10) if fp16x2_solve else ""}{"#define TW_DEVICE_ENV_BASIC" + chr(10) if basic else ""}#include "{header}"\n'
            f'{"TW_DEVICE_ENV_WIDE_SEARCH" if wide_search else "TW_DEVICE_ENV_SEARCH" if search else "TW_DEVICE_ENV"}({type_name}, {name})\n')
    deps = [header] + HEADERS + sorted(glob.glob(os.path.join(ROOT, "include", "*.hpp")))
    if not force and os.path.exists(src) and open(src).read() == text and not _stale(so, deps + [src]) and os.path.exists(asm):
        return so
    with open(src, "w") as f:
        f.write(text)
    tmp = so + f".{os.getpid()}.tmp"
    cmd = [hipcc(), *FLAGS, "-shared", "-save-temps=obj", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-I", os.path.dirname(header),
           src, "-o", tmp]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, cwd=out_dir)
    # -save-temps=obj: the gfx950 assembly goes next to the module, the other intermediates go
    base = os.path.basename(tmp)
    for f in os.listdir(out_dir):
        if not (f.startswith(base + "-") or f.startswith(stem + "-") or f.startswith(stem + ".hip-") or f.startswith(base + ".")) or f == base:
            continue
        p = os.path.join(out_dir, f)
        if f.endswith("-hip-amdgcn-amd-amdhsa-gfx950.s"):
            os.replace(p, asm)
        elif os.path.isfile(p) and not f.endswith((".so", ".hip")):
            os.remove(p)
    if r.returncode != 0:
        if os.path.exists(tmp):
            os.remove(tmp)
        raise RuntimeError(f"hipcc failed on the device environment {type_name} ({header}):\n{r.stdout}")
    if not os.path.exists(asm):
        os.remove(tmp)
        raise RuntimeError(f"build_device_env: no device assembly for {name}")
    try:
        _scan_asm([asm], f"the device environment module {name}")
    except RuntimeError:
        os.remove(tmp)
        raise
    os.replace(tmp, so)
    return so


def build_c_example() -> str:
    """examples/collect_from_c.c: a compiled host over the C ABI alone (gcc, links the library built above)."""
    src = os.path.join(ROOT, "examples", "collect_from_c.c")
    exe = os.path.join(ROOT, "examples", "collect_from_c")
    if _stale(exe, [src, LIB_PATH, os.path.join(ROOT, "include", "twisterl_hip.h")]):
        cmd = ["gcc", "-O2", "-Wall", "-I", os.path.join(ROOT, "include"), src, "-L", LIB_DIR, "-ltwisterl_hip",
               "-Wl,-rpath," + LIB_DIR, "-Wl,-rpath,$ORIGIN/../twisterl_amd/lib", "-lm", "-o", exe]
        if ABLATE or VARIANT:
            # the example links the PRODUCT library only: an instrumented or variant build neither builds nor uses it
            if not os.path.exists(exe):
                raise RuntimeError("examples/collect_from_c is built against the product library: run `python -m twisterl_amd.build` without TW_ABLATE / TW_VARIANT first")
            return exe
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"gcc failed on collect_from_c.c:\n{r.stdout}")
    return exe


if __name__ == "__main__":
    print(build_library(force="--force" in sys.argv, verbose=True))
    print(build_c_example())
