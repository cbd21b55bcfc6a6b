"""sha256 of the device-only assembly of every macarons_amd/csrc/*.hip: the check of a host-only change.

    python tools/device_asm_hash.py [--json OUT] [--against OTHER.json]

Each source is compiled with the library's own flags (build.FLAGS minus -shared -fPIC, plus the file's MCR_HIPCC_FLAGS line), device side
only, to assembly (--cuda-device-only -S); -fuse-cuid=none keeps the hash of the source text out of the symbol names, so two trees whose
device code is the same give the same bytes.  Needs hipcc, no GPU.  Run it at both commits and compare (--against exits 1 on a difference).
"""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from macarons_amd import build as b  # noqa: E402


def asm_hash(src):
    cmd = [b.hipcc_path()] + [f for f in b.FLAGS if f not in ("-shared", "-fPIC")] + b.per_file_flags(src) + \
          ["--cuda-device-only", "-S", "-fuse-cuid=none", "-I", b.CSRC, src, "-o", "-"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr.decode()}")
    assert not re.search(rb"__hip_cuid_[0-9a-f]", r.stdout), f"{src}: a hash of the source text is left in the symbol names"
    return hashlib.sha256(r.stdout).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--against")
    a = ap.parse_args()
    srcs = b.sources()
    with ThreadPoolExecutor(8) as ex:
        out = dict(zip((os.path.basename(s) for s in srcs), ex.map(asm_hash, srcs)))
    for k, v in out.items():
        print(f"{v}  {k}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    if a.against:
        with open(a.against) as f:
            other = json.load(f)
        bad = sorted(k for k in set(out) | set(other) if out.get(k) != other.get(k))
        print("device code differs in: " + ", ".join(bad) if bad else "device code identical in all %d files" % len(out))
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
