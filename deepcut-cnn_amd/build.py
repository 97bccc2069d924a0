"""Build libdeepcut_hip.so (HIP kernels + C-ABI) for gfx950, in-tree.

    python deepcut-cnn_amd/build.py [--force]

hipcc cross-compiles for gfx950 without a GPU, so this runs in the CPU-only build container; the
resulting .so travels to the GPU box with the repo snapshot (it is git-ignored, not gpurun-ignored).
"""
import hashlib
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "lib", "libdeepcut_hip.so")
# (the three gather-GEMM instantiation files take the longest by far: they come first, so that they start first)
SOURCES = ["conv_gemm_f16.hip", "conv_gemm_bf16.hip", "conv_gemm_f32.hip", "wino_f32.hip", "wino43_f32.hip", "wino_f16.hip", "stream1x1.hip", "stem_f16.hip",
           "stream1x1_f32.hip", "people.hip", "track.hip", "sparse_head.hip", "layers.hip", "pose.hip", "image_prep.hip", "draw.hip", "heat.hip", "redact.hip", "appearance.hip", "overlay.hip", "label.hip", "conv_gemm.cpp", "forms.cpp", "formats.cpp",
           "hdf5_reader.cpp", "runtime.cpp", "net_init.cpp", "net_lower.cpp", "net_tune.cpp", "net_run.cpp", "net_image.cpp", "net_group.cpp",
           "people.cpp", "track.cpp", "draw.cpp", "heat.cpp", "redact.cpp", "appearance.cpp", "overlay.cpp", "label.cpp", "sparse_pairwise.cpp", "streams.cpp", "multi_gpu.cpp", "c_api.cpp"]
HEADERS = ["formats.h", "net.h", "net_internal.h", "kernels.h", "kernel_prims.h", "conv_gemm.h", "conv_gemm_variants.h", "by_kind.h", "frame_tile.h", "tile_bins.h", "label_font.h", "label_tile.h",
           os.path.join("..", "..", "include", "deepcut_hip.h")]
MAX_JOBS = 16  # compiler processes at a time


KERNEL_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-inline-asm"]
# the sources whose kernels issue inline-asm memory requests (dc_dma16, dc_load_f32_untracked: the gather-GEMM), and what they include
ASM_SOURCES = ["conv_gemm_f16.hip", "conv_gemm_bf16.hip", "conv_gemm_f32.hip"]
ASM_HEADERS = ["conv_gemm.h", "conv_gemm_variants.h", "kernels.h", "kernel_prims.h"]


def _asm_path(src):
    return os.path.join(HERE, "lib", src[:-len(".hip")] + ".gfx950.s")


def _asm_key(src):
    """What the device assembly of a source depends on: the source and its headers, the flags, the compiler."""
    h = hashlib.sha256()
    for f in [src] + ASM_HEADERS:
        h.update(open(os.path.join(CSRC, f), "rb").read())
    h.update(" ".join(KERNEL_FLAGS).encode())
    h.update(_hipcc_version())
    return h.hexdigest()


def _asm_fresh(src):
    try:
        return os.path.getsize(_asm_path(src)) > 0 and open(_asm_path(src) + ".key").read().strip() == _asm_key(src)
    except OSError:
        return False


def _asm_cmd(src):
    """The command that writes the gfx950 assembly of a source (device side only, the library's own flags): what
    tools/check_asm_hazards.py reads.  build_lib runs it beside the object compiles so that the CPU test suite
    (tests/test_asm_hazards.py) finds the assemblies ready instead of compiling the gather-GEMM instantiations a second time."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    asm = _asm_path(src)
    os.makedirs(os.path.dirname(asm), exist_ok=True)
    for f in (asm, asm + ".key"):
        if os.path.exists(f):
            os.remove(f)
    return [hipcc] + KERNEL_FLAGS + ["--offload-device-only", "-S", os.path.join(CSRC, src), "-o", asm + ".tmp"]


def _write_key(path, key):
    with open(path + ".key", "w") as f:
        f.write(key + "\n")


def _asm_finish(src, key):
    os.replace(_asm_path(src) + ".tmp", _asm_path(src))
    _write_key(_asm_path(src), key)


def _run(cmds):
    """Run the commands, MAX_JOBS at a time; their exit codes, in order."""
    with ThreadPoolExecutor(MAX_JOBS) as pool:
        return list(pool.map(subprocess.call, cmds))


def device_asm():
    """Paths of the gfx950 assemblies of ASM_SOURCES, each compiled now unless the cached one matches its sources."""
    stale = [(s, _asm_key(s)) for s in ASM_SOURCES if not _asm_fresh(s)]
    for (src, key), code in zip(stale, _run([_asm_cmd(s) for s, _ in stale])):
        if code != 0:
            raise RuntimeError("device assembly of %s failed" % src)
        _asm_finish(src, key)
    return [_asm_path(s) for s in ASM_SOURCES]


_HIPCC_VERSION = None


def _hipcc_version():
    global _HIPCC_VERSION
    if _HIPCC_VERSION is None:
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        try:
            out = subprocess.run([hipcc, "--version"], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL).stdout
            # the compiler's identity only: the version lines.  (The rest of the output names the host — `InstalledDir`, configuration
            # files, on a GPU box the detected agents — and would make the prebuilt library look stale on the box it travels to.)
            _HIPCC_VERSION = b"\n".join(ln for ln in out.splitlines() if b"version" in ln.lower())
        except OSError:
            _HIPCC_VERSION = b""
    return _HIPCC_VERSION


def _obj_key(src):
    """What an object depends on, by CONTENT: its source, every header, the flags, the compiler.  (Round 5 compared mtimes: a checkout
    that rewinds sources under a newer .so shipped a stale library silently — the .so travels prebuilt to the GPU box.)"""
    h = hashlib.sha256()
    for f in [src] + HEADERS:
        h.update(f.encode() + b"\0")
        h.update(open(os.path.join(CSRC, f), "rb").read())
    h.update(" ".join(KERNEL_FLAGS).encode())
    h.update(_hipcc_version())
    return h.hexdigest()


def _lib_key(keys):
    return hashlib.sha256("\n".join(keys).encode()).hexdigest()


def _read(path):
    try:
        return open(path).read().strip()
    except OSError:
        return None


def _stale():
    if not os.path.exists(OUT):
        return True
    return _read(OUT + ".key") != _lib_key([_obj_key(s) for s in SOURCES])


def build_lib(force=False, verbose=True):
    """Per-file incremental, keyed by content hashes (a gather-GEMM instantiation file takes a minute, the other translation units
    seconds each — they compile in parallel, MAX_JOBS at a time): an object is rebuilt when the hash of its source + the headers + the
    flags + the compiler differs from the one recorded beside it, the library is re-linked when any object's key changed."""
    if not force and not _stale():
        return OUT
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    objs, keys = [], []
    jobs = []  # (what, command, what to do once it has succeeded)
    for src in SOURCES:
        obj = os.path.join(HERE, "lib", src + ".o")
        objs.append(obj)
        key = _obj_key(src)
        keys.append(key)
        sp = os.path.join(CSRC, src)
        if not force and os.path.exists(obj) and _read(obj + ".key") == key:
            continue
        if os.path.exists(obj + ".key"):
            os.remove(obj + ".key")
        cmd = [hipcc] + KERNEL_FLAGS + ["-Wall", "-Wno-unused-function", "-c", sp, "-o", obj]
        if src.endswith(".cpp"):
            cmd.insert(1, "-x")
            cmd.insert(2, "hip")
        if verbose:
            print(" ".join(cmd), flush=True)
        jobs.append((src, cmd, lambda obj=obj, key=key: _write_key(obj, key)))
        if src in ASM_SOURCES and not _asm_fresh(src):
            jobs.append(("device assembly of " + src, _asm_cmd(src), lambda src=src, key=_asm_key(src): _asm_finish(src, key)))
    failed = []
    for (what, _, done), code in zip(jobs, _run([j[1] for j in jobs])):
        if code != 0:
            failed.append(what)
        else:
            done()
    if failed:
        raise RuntimeError("compilation failed: %s" % ", ".join(failed))
    if os.path.exists(OUT + ".key"):
        os.remove(OUT + ".key")
    cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", OUT] + objs
    if verbose:
        print(" ".join(cmd), flush=True)
    subprocess.check_call(cmd)
    _write_key(OUT, _lib_key(keys))
    return OUT


if __name__ == "__main__":
    print(build_lib(force="--force" in sys.argv))
