#!/usr/bin/env python3
"""Code footprint of the decode kernels (profiles/prologue_fetch.md): per production instantiation the bytes of the whole kernel and the bytes from its entry
to the chain wave's main-loop marker -- the span a cold launch fetches on its critical path before the first add.

The numbers come from the gfx950 code object, either the one of a -save-temps build of csrc/lnb_kernels.hip (tools/isa_audit.py compile_to_asm, what
tests/test_isa_audit.py builds: `--build`, or `--dir` of such a build) or the one inside the built library (default: liblnb_hip.so's fat binary).
Totals are the ELF symbol sizes; the marker is found in the disassembly:
  gemv_quad_kernel, rowcast_lds_kernel   the `s_setprio 3` in front of the chain waves' main loop
  gemv_chain_pk_kernel                   the first v_pk_add_f32 (only the chain wave's main loop has one)
A kernel whose last template argument is `true` where production's is `false` is its TIMING instantiation (stamps, timed barriers), listed beside it.

usage: tools/code_footprint.py [--build | --dir DIR | --so PATH] [--all]
"""
import os
import re
import struct
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/llvm/bin"
SO = os.path.join(ROOT, "llama-nuts-and-bolts_amd", "liblnb_hip.so")

# the launches of one 8B decode token (mangled prefix up to the TIMING argument, marker); EPI: 1 QKV_ROPE, 2 RESID, 3 SILU_MUL, 4 STORE2
PRODUCTION = [
    ("wq|wk|wv   gemv_quad_kernel<24,256,6,5,QKV_ROPE,true,2>", "_Z16gemv_quad_kernelILi24ELi256ELi6ELi5ELi1ELb1ELi2E", r"s_setprio 3"),
    ("wo, w2     rowcast_lds_kernel<RESID>", "_Z18rowcast_lds_kernelILi2E", r"s_setprio 3"),
    ("gate|up    gemv_chain_pk_kernel<56,2,28672,7,5,SILU_MUL,true,2>", "_Z20gemv_chain_pk_kernelILi56ELi2ELi28672ELi7ELi5ELi3ELb1ELi2E", r"v_pk_add_f32"),
    ("head       gemv_chain_pk_kernel<64,2,32768,8,5,STORE2,true,2>", "_Z20gemv_chain_pk_kernelILi64ELi2ELi32768ELi8ELi5ELi4ELb1ELi2E", r"v_pk_add_f32"),
]
# every kernel family that has a TIMING instantiation (the decode kernels)
DECODE_FAMILIES = ("gemv_chain_kernel", "gemv_chain_pk_kernel", "gemv_quad_kernel", "rowcast_kernel", "rowcast_lds_kernel", "attn_exact_kernel",
                   "attn_long_pv_kernel", "attn_long_pv2_kernel")
CLOCK_READS = ("s_memtime", "s_memrealtime")


def code_objects_of_library(so=SO):
    """the gfx950 code objects inside a shared library's .hip_fatbin section (uncompressed clang offload bundles)"""
    with tempfile.TemporaryDirectory() as wd:
        fat = os.path.join(wd, "fat.bin")
        subprocess.check_call([os.path.join(LLVM, "llvm-objcopy"), "-O", "binary", "--only-section=.hip_fatbin", so, fat])
        data = open(fat, "rb").read()
    magic, out = b"__CLANG_OFFLOAD_BUNDLE__", []
    for m in re.finditer(re.escape(magic), data):
        base = m.start()
        n, = struct.unpack_from("<Q", data, base + len(magic))
        at = base + len(magic) + 8
        for _ in range(n):
            off, size, tl = struct.unpack_from("<QQQ", data, at)
            triple = data[at + 24:at + 24 + tl].decode()
            at += 24 + tl
            if "gfx950" in triple and size:
                out.append(data[base + off:base + off + size])
    if not out:
        raise RuntimeError("no gfx950 code object in %s (a compressed fat binary? build with --build instead)" % so)
    return out


def code_object_of_dir(d):
    for f in sorted(os.listdir(d)):
        if f.endswith("gfx950.out"):
            return open(os.path.join(d, f), "rb").read()
    raise RuntimeError("no gfx950 code object in %s" % d)


def kernels_of(obj):
    """{mangled kernel name: (bytes, [(offset from entry, instruction text)])} of the decode families of one code object"""
    with tempfile.TemporaryDirectory() as wd:
        path = os.path.join(wd, "k.co")
        open(path, "wb").write(obj)
        syms = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-sW", path], capture_output=True, text=True, check=True).stdout
        dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", path], capture_output=True, text=True, check=True).stdout
    fam = re.compile(r"^_Z\d+(?:%s)I" % "|".join(DECODE_FAMILIES))
    size = {}
    for ln in syms.split("\n"):
        f = ln.split()
        if len(f) >= 8 and f[3] == "FUNC" and fam.match(f[7]):
            size[f[7]] = int(f[2])
    out, cur, entry = {}, None, 0
    for ln in dis.split("\n"):
        m = re.match(r"^([0-9a-f]+) <(\S+)>:", ln)
        if m:
            cur = m.group(2) if m.group(2) in size else None
            entry = int(m.group(1), 16)
            if cur:
                out[cur] = (size[cur], [])
            continue
        if cur and ln.startswith("\t"):
            m = re.match(r"^\t(.*?)\s*// ([0-9A-Fa-f]+):", ln)
            if m:
                out[cur][1].append((int(m.group(2), 16) - entry, m.group(1)))
    return out


def is_timing(name):
    """the TIMING instantiation of a decode kernel: its last template argument is `true` and the same name with `false` exists or is production's form"""
    return bool(re.search(r"Lb1EEv\d+(?:Gemv|Attn)Params$", name)) and timing_partner(name) is not None


def timing_partner(name):
    m = re.match(r"^(.*)Lb1E(Ev\d+(?:Gemv|Attn)Params)$", name)
    return m.group(1) + "Lb0E" + m.group(2) if m else None


def load(argv):
    if "--build" in argv:
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import isa_audit
        with tempfile.TemporaryDirectory() as wd:
            isa_audit.compile_to_asm(wd)
            objs = [code_object_of_dir(wd)]
    elif "--dir" in argv:
        objs = [code_object_of_dir(argv[argv.index("--dir") + 1])]
    else:
        objs = code_objects_of_library(argv[argv.index("--so") + 1] if "--so" in argv else SO)
    ks = {}
    for o in objs:
        ks.update(kernels_of(o))
    return ks


def footprint(ks):
    """[(label, variant, total bytes, bytes from entry to the main-loop marker)] of the production decode kernels and their TIMING instantiations"""
    rows = []
    for label, prefix, marker in PRODUCTION:
        for variant, tail in (("production", ("E", "Lb0EE")), ("timing", ("Lb1EE",))):
            names = [n for n in ks if any(re.fullmatch(re.escape(prefix + t) + r"v\d+GemvParams", n) for t in tail)]
            for n in names:
                total, ins = ks[n]
                at = next((off for off, t in ins if re.match(marker, t)), None)
                rows.append((label, variant, total, at))
    return rows


def main(argv):
    ks = load(argv)
    print("%-64s %-10s %8s %10s" % ("kernel", "variant", "bytes", "to marker"))
    for label, variant, total, at in footprint(ks):
        print("%-64s %-10s %8d %10s" % (label, variant, total, "-" if at is None else "0x%x = %d" % (at, at)))
    if "--all" in argv:
        for n in sorted(ks):
            clk = sum(1 for _, t in ks[n][1] if t.split()[0] in CLOCK_READS)
            print("%8d  clock reads %3d  %s%s" % (ks[n][0], clk, "[timing] " if is_timing(n) and timing_partner(n) in ks else "", n))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
