"""sha256 of the device-only assembly of every macarons_amd/csrc/*.hip: the check of a host-only change.

    python tools/device_asm_hash.py [--per-kernel [--ignore-file]] [--json OUT] [--against OTHER.json]

Each source is compiled with the library's own flags (build.FLAGS minus -shared -fPIC, plus the file's MCR_HIPCC_FLAGS line), device side
only, to assembly (--cuda-device-only -S); -fuse-cuid=none keeps the hash of the source text out of the symbol names, so two trees whose
device code is the same give the same bytes.  Needs hipcc, no GPU.  Run it at both commits and compare (--against exits 1 on a difference).

--per-kernel: one hash per global function instead of one per file, for a change that deletes a kernel (every function behind the
deleted one gets another ordinal, so the file's bytes differ although no surviving kernel changed).  A function is the text from its
`.globl SYM` to its `.Lfunc_endN:` (the .amdhsa_kernel block lies in between); comments (`;` to the end of the line) and trailing
blanks are dropped and the function's ordinal in `BB<N>_` and `.Lfunc_begin<N>` / `.Lfunc_end<N>` is replaced before hashing.  Against
another --per-kernel file, symbols that are gone are listed; a symbol that differs or is new exits 1.

--ignore-file (with --per-kernel --against): compare by symbol alone, for a change that moves kernels between files (a moved kernel
would else show as gone plus new); a symbol that occurs in two files of either tree is an error.
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


def per_kernel_hashes(asm):
    """{symbol: sha256 of its normalised text} for every `.globl SYM` ... `.Lfunc_endN:` stretch of the assembly."""
    out, sym, lines = {}, None, []
    for line in asm.decode().splitlines():
        m = re.match(r"\s*\.globl\s+(\S+)", line)
        if m:
            sym, lines = m.group(1), []
        if sym is None:
            continue
        line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1#", re.sub(r"BB\d+_", "BB#_", line.split(";", 1)[0].rstrip()))
        lines.append(line)
        if re.match(r"\.Lfunc_end#:", line):
            out[sym] = hashlib.sha256("\n".join(lines).encode()).hexdigest()
            sym = None
    return out


def asm_hash(src, per_kernel=False):
    cmd = [b.hipcc_path()] + [f for f in b.FLAGS if f not in ("-shared", "-fPIC")] + b.per_file_flags(src) + \
          ["--cuda-device-only", "-S", "-fuse-cuid=none", "-I", b.CSRC, src, "-o", "-"]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed for {src}:\n{r.stderr.decode()}")
    assert not re.search(rb"__hip_cuid_[0-9a-f]", r.stdout), f"{src}: a hash of the source text is left in the symbol names"
    return per_kernel_hashes(r.stdout) if per_kernel else hashlib.sha256(r.stdout).hexdigest()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json")
    ap.add_argument("--against")
    ap.add_argument("--per-kernel", action="store_true")
    ap.add_argument("--ignore-file", action="store_true")
    a = ap.parse_args()
    srcs = b.sources()
    with ThreadPoolExecutor(8) as ex:
        out = dict(zip((os.path.basename(s) for s in srcs), ex.map(lambda s: asm_hash(s, a.per_kernel), srcs)))
    for k, v in out.items():
        print(f"{len(v)} functions  {k}" if a.per_kernel else f"{v}  {k}")
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)
    if a.against:
        with open(a.against) as f:
            other = json.load(f)
        if a.per_kernel:
            flat = lambda d: {(k, sym): h for k, v in d.items() for sym, h in v.items()}
            if a.ignore_file:                       # by symbol alone: a kernel may have moved to another file, but must not exist twice
                for d in (out, other):
                    syms = [sym for v in d.values() for sym in v]
                    twice = sorted({s for s in syms if syms.count(s) > 1})
                    if twice:
                        sys.exit("--ignore-file: in two files: " + ", ".join(twice))
                flat = lambda d: {("*", sym): h for v in d.values() for sym, h in v.items()}
            mine, theirs = flat(out), flat(other)
            gone = sorted(set(theirs) - set(mine))
            bad = sorted(k for k in mine if mine[k] != theirs.get(k))
            for k, sym in gone:
                print(f"gone: {k}  {sym}")
            for k, sym in bad:
                print(f"{'differs' if (k, sym) in theirs else 'new'}: {k}  {sym}")
            print(f"{len(mine) - len(bad)} of {len(mine)} functions identical, {len(gone)} gone, {len(bad)} differ or are new")
            sys.exit(1 if bad else 0)
        bad = sorted(k for k in set(out) | set(other) if out.get(k) != other.get(k))
        print("device code differs in: " + ", ".join(bad) if bad else "device code identical in all %d files" % len(out))
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
