"""Build libmi355rtdetr.so (gfx950) in-tree with hipcc.  `python -m telescope_cam_detection_amd.build`.

hipcc cross-compiles without a GPU; the .so is git-ignored but travels to the GPU box with the
repo snapshot.  A rebuild happens only when a source is newer than the library.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

PKG = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG, "csrc")
LIB_DIR = os.path.join(PKG, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libmi355rtdetr.so")
SOURCES = ["conv_igemm.hip", "ops.hip", "decoder.hip", "engine.hip", "testapi.hip", "motion.hip", "mog2.hip", "jpeg.hip", "overlay.hip", "enhance.hip", "esrgan.hip", "ingest.hip", "facemask.hip", "classifier.hip", "yolox_post.hip", "yolox_net.hip"]
HEADERS = [os.path.join(CSRC, "common.h"), os.path.join(CSRC, "error.h"), os.path.join(CSRC, "backend.h"), os.path.join(CSRC, "call_parts.h"), os.path.join(CSRC, "global_bytes.h"), os.path.join(CSRC, "engine_internal.h"), os.path.join(CSRC, "gauss8.h"), os.path.join(CSRC, "gauss_taps.h"), os.path.join(CSRC, "enhance_tables.h"), os.path.join(CSRC, "weight_blob.h"), os.path.join(CSRC, "net_plan.h"), os.path.join(CSRC, "esrgan_host.h"), os.path.join(CSRC, "ingest_host.h"), os.path.join(CSRC, "resize_taps.h"), os.path.join(CSRC, "facemask_host.h"), os.path.join(CSRC, "classifier_host.h"), os.path.join(CSRC, "yolox_post_host.h"), os.path.join(CSRC, "yolox_net_host.h"), os.path.join(os.path.dirname(PKG), "include", "rtdetr_mi355.h"),
           os.path.join(os.path.dirname(PKG), "include", "rtdetr_mi355_test.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wall", "-Wno-unused-function"]


def _hipcc() -> str:
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found (needs the ROCm toolchain)")


def needs_build() -> bool:
    if not os.path.exists(LIB_PATH):
        return True
    t = os.path.getmtime(LIB_PATH)
    deps = [os.path.join(CSRC, s) for s in SOURCES] + HEADERS
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = True) -> str:
    if not force and not needs_build():
        return LIB_PATH
    hipcc = _hipcc()
    os.makedirs(LIB_DIR, exist_ok=True)
    obj_dir = os.path.join(LIB_DIR, "obj")
    os.makedirs(obj_dir, exist_ok=True)

    # which headers a source includes: an object is rebuilt only when its source or one of THOSE headers is newer (conv_igemm.hip alone
    # takes minutes; engine / testapi / decoder / ops seconds)
    common = [os.path.join(CSRC, "common.h"), os.path.join(CSRC, "error.h")]
    deps_of = {src: (HEADERS if src in ("engine.hip", "testapi.hip", "motion.hip", "mog2.hip", "jpeg.hip", "overlay.hip", "enhance.hip", "esrgan.hip", "ingest.hip", "facemask.hip", "classifier.hip", "yolox_post.hip", "yolox_net.hip") else common) for src in SOURCES}   # only the host side sees the ABI headers

    def compile_one(src):
        obj = os.path.join(obj_dir, src.replace(".hip", ".o"))
        path = os.path.join(CSRC, src)
        if not force and os.path.exists(obj) and all(os.path.getmtime(d) <= os.path.getmtime(obj) for d in [path] + deps_of[src]):
            return obj
        cmd = [hipcc, *FLAGS, "-c", path, "-o", obj]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError(f"hipcc failed on {src}:\n{r.stderr[-4000:]}")
        if verbose and r.stderr.strip():
            print(r.stderr[-2000:], file=sys.stderr)
        return obj

    with ThreadPoolExecutor(max_workers=5) as ex:
        objs = list(ex.map(compile_one, SOURCES))
    tmp = LIB_PATH + ".tmp"
    r = subprocess.run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", tmp, *objs], capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"link failed:\n{r.stderr[-4000:]}")
    # -shared accepts undefined symbols: a kernel whose host stub was not emitted (seen with ROCm 7.2 on a kernel template holding a
    # dependent-extent array captured by a lambda) only fails at dlopen on the GPU box.  Refuse to ship such a library.
    nm = shutil.which("nm")
    if nm:
        u = subprocess.run([nm, "-C", "--undefined-only", tmp], capture_output=True, text=True).stdout
        bad = [l.strip() for l in u.splitlines() if "rtd::" in l or "rtd_eng::" in l or "__device_stub__" in l]
        if bad:
            os.remove(tmp)
            raise RuntimeError("libmi355rtdetr.so would have unresolved kernel symbols:\n" + "\n".join(bad[:10]))
    os.replace(tmp, LIB_PATH)
    if verbose:
        print(f"built {LIB_PATH}")
    return LIB_PATH


if __name__ == "__main__":
    build(force="--force" in sys.argv)
