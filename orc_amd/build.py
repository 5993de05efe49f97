"""Build liborcgpu.so in-tree with hipcc for gfx950 (no JIT cache: the .so
travels to the GPU box with the repo snapshot)."""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
# ORCG_PHASE_PROF=1 builds the phase-profiling variant (kernel cycle counters,
# scripts/phase_prof.py) as liborcgpu_prof.so next to the product library.
PROF = os.environ.get("ORCG_PHASE_PROF", "") == "1"
# ORCG_AB=1 builds the A/B variant (the device copy probes of
# probe_kernels.hip, scripts/ab_rlev2.py --refs probe5) as liborcgpu_ab.so.
AB = os.environ.get("ORCG_AB", "") == "1"
OUT = os.path.join(HERE, "liborcgpu_prof.so" if PROF else ("liborcgpu_ab.so" if AB else "liborcgpu.so"))
OBJ = os.path.join(HERE, "build_prof" if PROF else ("build_ab" if AB else "build"))
ARCH = os.environ.get("ORCG_OFFLOAD_ARCH", "gfx950")

SOURCES = ["rlev2_kernels.hip", "rlev2_tiled_inst_serial.hip", "rlev2_tiled_inst_dense.hip", "rlev2_tiled_inst_union.hip", "rlev2_tiled.cpp", "rlev2_expand.hip", "byterle_kernels.hip", "column_kernels.hip", "rlev1_kernels.hip", "decimal_kernels.hip", "convert_kernels.hip", "arrow_kernels.hip", "inflate_kernels.hip", "filter_kernels.hip", "orcg_ctx.cpp", "pinned.cpp", "host_plan.cpp", "rlev2_route.cpp", "inflate_plan.cpp", "inflate_api.cpp", "filter_plan.cpp", "filter_api.cpp", "host_decode.cpp", "rlev2_api.cpp", "debug_api.cpp",
           "multi_launch.cpp", "rlev1_api.cpp", "orc_file.cpp", "reader_api.cpp", "reader_prepare.cpp",
           "reader_collect.cpp", "reader_streams.cpp", "reader_decode.cpp", "reader_fork.cpp", "reader_stripes.cpp",
           "row_reader.cpp", "byterle_api.cpp", "decimal_api.cpp", "convert_api.cpp", "arrow_api.cpp", "arrow_export.cpp", "timezone.cpp", "encoder.cpp", "java_face.cpp"]
if PROF or AB:
    SOURCES.append("probe_kernels.hip")

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ["-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function", "-Wno-unused-result", "-Wno-unused-value"]
if PROF:
    FLAGS.append("-DORCG_PHASE_PROF")
if PROF or AB:
    # experiment knobs of the A/B build (e.g. ORCG_AB_FLAGS="-DORCG_ITEM_MAX=1")
    FLAGS.extend(os.environ.get("ORCG_AB_FLAGS", "").split())


def _mtime(p):
    return os.path.getmtime(p) if os.path.exists(p) else 0.0


def stale(obj, src, dep, tools=(os.path.abspath(__file__),)):
    """Whether `obj` has to be compiled again: it is missing, it has no
    dependency file `dep` (the compiler's -MD output, make syntax) yet, or its
    source, a file that `dep` names or one of `tools` is missing or not older
    than it."""
    if not os.path.exists(obj) or not os.path.exists(dep):
        return True
    with open(dep) as f:
        words = f.read().replace("\\\n", " ").split()
    deps = [w for w in words if not w.endswith(":")]  # (the rule's target ends in a colon)
    built = os.path.getmtime(obj)
    return any(not os.path.exists(p) or os.path.getmtime(p) >= built for p in [src, *tools, *deps])


def build(force=False, verbose=False):
    os.makedirs(OBJ, exist_ok=True)
    objs, cmds = [], []
    for s in SOURCES:
        src = os.path.join(CSRC, s)
        obj = os.path.join(OBJ, s + ".o")
        objs.append(obj)
        if not force and not stale(obj, src, obj + ".d"):
            continue
        cmd = [HIPCC] + FLAGS + ["-MD", "-MF", obj + ".d", "-c", src, "-o", obj]
        if s.endswith(".hip"):
            cmd[1:1] = ["-x", "hip", "--offload-arch=" + ARCH]
        else:
            cmd[1:1] = ["-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include"]
        cmds.append(cmd)
    # translation units compile in parallel (the slowest, the rlev2_tiled instance units, first)
    cmds.sort(key=lambda c: "rlev2_tiled_inst_" not in c[-3])
    from concurrent.futures import ThreadPoolExecutor

    def run(cmd):
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)

    jobs = max(1, min(len(cmds), int(os.environ.get("MAX_JOBS", "8") or 8), os.cpu_count() or 1))
    with ThreadPoolExecutor(jobs) as ex:
        for f in [ex.submit(run, c) for c in cmds]:
            f.result()
    if force or _mtime(OUT) < max(_mtime(o) for o in objs):
        cmd = [HIPCC, "-shared", "-fPIC", "-o", OUT] + objs + ["-Wl,-soname," + os.path.basename(OUT), "-lz", "-ldl", "-lpthread"]
        if verbose:
            print(" ".join(cmd), file=sys.stderr)
        subprocess.check_call(cmd)
    return OUT


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
