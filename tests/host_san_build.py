"""Build tests/host_san/driver.cpp, which includes gypsum_hip.hip itself, into two sanitizer programs under tests/host_san/_build/:

    asan_ubsan   -fsanitize=address,undefined -fno-sanitize-recover=undefined
    tsan         -fsanitize=thread

    python tests/host_san_build.py [--force]

The host code is compiled with exactly the driver's flags.  The driver never launches a kernel, so the device pass (almost all of a
full compile of this translation unit: about three minutes) is left out: `--offload-host-only` compiles the host side alone, which
leaves one undefined symbol, the `__hip_fatbin_<hash>` blob the registration stub points at.  A page of zeros under that name
satisfies the linker; the HIP runtime only records the pointer at start-up and would parse it on the first kernel launch, which
never comes.  About 35 s per program instead of 3 min, and the two are built side by side.

Builds are keyed by a sha256 over the flags, the driver and every file gypsum_amd/build.py lists as SOURCES + HEADERS: a second run
builds nothing.  libgypsum_hip.so and its stamp are not touched.
"""
from __future__ import annotations

import hashlib
import re
import subprocess
import sys
import time
from pathlib import Path

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
from gypsum_amd.build import HEADERS, SOURCES, find_hipcc  # noqa: E402

DRIVER = HERE / "host_san" / "driver.cpp"
OUT = HERE / "host_san" / "_build"
COMMON = ["--offload-arch=gfx950", "--offload-host-only", "-O1", "-g", "-std=c++17", "-DGYP_FOR_EACH_RATE(X)=X(8)",
          "-Xarch_host", "-fno-omit-frame-pointer", "-Wno-unused-result", "-Wno-unused-value"]
PROGRAMS = {
    "asan_ubsan": ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined", "-DGYP_DRIVER_UBSAN"],
    "tsan": ["-Xarch_host", "-fsanitize=thread"],
}
BANNER = {"asan_ubsan": "sanitizers: address undefined", "tsan": "sanitizers: thread"}


def key(name: str) -> str:
    h = hashlib.sha256()
    h.update(" ".join(COMMON + PROGRAMS[name]).encode())
    for p in [DRIVER, Path(__file__), *sorted(SOURCES + HEADERS)]:
        h.update(p.name.encode())
        h.update(p.read_bytes())
    return h.hexdigest()


def program(name: str) -> Path:
    return OUT / name


def is_stale(name: str) -> bool:
    stamp = OUT / f"{name}.key"
    return not program(name).exists() or not stamp.exists() or stamp.read_text().strip() != key(name)


def build_one(name: str) -> None:
    OUT.mkdir(parents=True, exist_ok=True)
    hipcc = find_hipcc()
    digest = key(name)
    obj, stub = OUT / f"{name}.o", OUT / f"{name}_fatbin.c"
    flags = COMMON + PROGRAMS[name]
    subprocess.run([hipcc, *flags, "-x", "hip", "-c", str(DRIVER), "-o", str(obj)], check=True, cwd=str(HERE))
    blobs = sorted(set(re.findall(rb"__hip_fatbin_[0-9a-f]{8,}", obj.read_bytes())))
    if len(blobs) != 1:
        raise RuntimeError(f"expected one __hip_fatbin_<hash> symbol in {obj}, found {blobs}")
    stub.write_text(f"const char {blobs[0].decode()}[4096] __attribute__((aligned(4096))) = {{0}};\n")
    link = [f for f in PROGRAMS[name] if f.startswith("-fsanitize=")]
    subprocess.run([hipcc, "--offload-arch=gfx950", *link, str(obj), "-x", "c", str(stub), "-o", str(program(name))], check=True, cwd=str(HERE))
    obj.unlink()
    (OUT / f"{name}.key").write_text(digest + "\n")


def build(force: bool = False) -> dict:
    """Returns {name: {"path": Path, "seconds": build time or 0.0 if cached}}; the stale programs are built in concurrent processes."""
    todo = [n for n in PROGRAMS if force or is_stale(n)]
    t0 = time.time()
    procs = {n: subprocess.Popen([sys.executable, str(Path(__file__)), "--one", n], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for n in todo}
    took = {}
    for n, p in procs.items():
        out, _ = p.communicate()
        took[n] = time.time() - t0
        if p.returncode != 0:
            raise RuntimeError(f"host sanitizer build '{n}' failed:\n{out[-4000:]}")
    return {n: {"path": program(n), "seconds": took.get(n, 0.0)} for n in PROGRAMS}


if __name__ == "__main__":
    if "--one" in sys.argv:
        build_one(sys.argv[sys.argv.index("--one") + 1])
    else:
        for n, r in build(force="--force" in sys.argv).items():
            print(f"{r['path']}  {r['seconds']:.0f} s")
