"""Build recipe for libartspeech_hip.so (hipcc, gfx950 only).  Idempotent: sources newer than their
object files are recompiled, then everything is linked in-tree next to this file."""
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "csrc", "build")
LIB = os.path.join(HERE, "libartspeech_hip.so")

ARCH = "gfx950"
COMMON = ["-O3", "-fPIC", "-std=c++17", f"-I{os.path.join(ROOT, 'include')}", f"-I{CSRC}"]
# per-file extra flags: metrics.hip keeps IEEE op-by-op arithmetic (arg-min pairs and the fp64 area
# function must be bit-reproducible), so no fused multiply-add contraction there; pc_eval.hip likewise (its denormalisation
# is torch's multiply, then add); p2cp_loss.hip finds its closest points with metrics.hip's arithmetic, so it is built alike;
# report.hip rounds x * scale before it centres it, like the reference's table in mm; contours.hip's results are selections
# and op-by-op float32 arithmetic ((p - u) + 0.3, (x - mean) / std), bit-equal to the reference's torch expressions;
# vocal_tract_tube.hip picks its junctions with metrics.hip's closest-point arithmetic and lerps as numpy does.
SOURCES = {
    "error.cpp": [],
    "prof.hip": [],
    "gemm_plan.cpp": [],
    "lin_plan.cpp": [],
    "gemm_f32.hip": [],
    "wgrad_f32.hip": [],
    "lin_f32.hip": [],
    "gemm_s6.hip": [],
    "rowops.hip": [],
    "gru.hip": [],
    "lstm.hip": [],
    "conv.hip": [],
    "scorer_wgrad.hip": [],
    "ctc.hip": [],
    "ctc_align.hip": [],
    "ctc_beam.hip": [],
    "recog_eval.hip": [],
    "frame_ce.hip": [],
    "attention.hip": [],
    "metrics.hip": ["-ffp-contract=off"],
    "p2cp_loss.hip": ["-ffp-contract=off"],
    "multi_mlp.hip": [],
    "pca.hip": [],
    "mean_contour.hip": [],
    "pc_eval.hip": ["-ffp-contract=off"],
    "report.hip": ["-ffp-contract=off"],
    "contours.hip": ["-ffp-contract=off"],
    "melspec.hip": [],
    "resample_plan.cpp": [],
    "resample.hip": [],
    "contour_spline.hip": [],
    "vocal_tract_tube.hip": ["-ffp-contract=off"],
    "vt_acoustics.hip": [],
    "vt_synth.hip": [],
    "tsne.hip": [],
    "artspeech.hip": [],
}


def _newer(src, dst, extra=()):
    if not os.path.exists(dst):
        return True
    t = os.path.getmtime(dst)
    return any(os.path.getmtime(s) > t for s in (src, *extra))


def resources_path(name):
    """Where the device compile of csrc/<name> leaves hipcc's per-kernel resource remarks (registers, scratch, occupancy)."""
    return os.path.join(OBJ, name.rsplit(".", 1)[0] + ".resources.txt")


def compile_one(name, extra, obj, hipcc, verbose=True):
    """One source to its object.  Device compiles ask for the kernel-resource-usage remarks (free: the numbers exist anyway) and
    keep them next to the object; whatever else the compiler says goes to stderr as usual."""
    src = os.path.join(CSRC, name)
    if name.endswith(".cpp"):
        cmd = [hipcc, *COMMON, "-c", src, "-o", obj]
        if verbose:
            print("[build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
        return
    cmd = [hipcc, f"--offload-arch={ARCH}", *COMMON, *extra, "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", obj]
    if verbose:
        print("[build]", " ".join(cmd), flush=True)
    r = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    remarks, rest, quoted = [], [], False
    for line in r.stderr.splitlines(keepends=True):
        if "[-Rpass-analysis=kernel-resource-usage]" in line:
            remarks.append(line)
            quoted = True
        elif quoted and re.match(r"\s+\d*\s*\|", line):
            continue             # the source line and caret clang quotes under a remark
        else:
            rest.append(line)
            quoted = False
    sys.stderr.write("".join(rest))
    if r.returncode:
        raise subprocess.CalledProcessError(r.returncode, cmd)
    with open(resources_path(name), "w") as f:
        f.writelines(remarks)


def build(force=False, verbose=True):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(OBJ, exist_ok=True)
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers.append(os.path.join(ROOT, "include", "artspeech_hip.h"))
    objs, relink = [], force
    for name, extra in SOURCES.items():
        src = os.path.join(CSRC, name)
        obj = os.path.join(OBJ, name.rsplit(".", 1)[0] + ".o")
        objs.append(obj)
        if force or _newer(src, obj, headers):
            compile_one(name, extra, obj, hipcc, verbose)
            relink = True
    if relink or not os.path.exists(LIB):
        cmd = [hipcc, f"--offload-arch={ARCH}", "-shared", "-fPIC", "-o", LIB, *objs]
        if verbose:
            print("[build]", " ".join(cmd), flush=True)
        subprocess.check_call(cmd)
    return LIB


if __name__ == "__main__":
    print(build(force="--force" in sys.argv))
