#!/usr/bin/env python3
"""Is the device code of two builds of csrc/ the same?  Needs no GPU.
  python3 tools/kernel_diff.py PARENT_BUILD_DIR CHANGE_BUILD_DIR [--moved OLD=NEW1,NEW2] [--rename REGEX=REPL ...] [--out FILE]
For every *.o of both directories the gfx950 code object is taken out of the fat binary (llvm-objcopy --dump-section .hip_fatbin,
clang-offload-bundler --unbundle).  Objects present under one name on both sides are compared by sha256.  For --moved OLD=NEW,...
the kernels of OLD.o are looked up in the NEW objects and compared symbol by symbol: the disassembled instruction text (addresses
and encodings dropped, so that a branch reads as its distance) and the resource record of the kernel descriptor
(.amdhsa_ directives of llvm-objdump's disassembly of the .rodata descriptor: VGPRs, SGPRs, LDS, scratch, kernel-argument size).
--rename REGEX=REPL (repeatable) rewrites the PARENT's symbol names before they are looked up: a kernel that gained a template parameter
has a new mangled name and is still compared instruction by instruction.
A plain per-symbol diff; exit status 1 if anything differs."""
import argparse, hashlib, os, re, subprocess, sys, tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def code_object(obj, tmp):
    """path of the gfx950 code object of a host object file, or None if it has no device code"""
    # named after the whole path: two build directories of the same name (parent/build, change/build) must not share a file
    tag = hashlib.sha256(os.path.abspath(obj).encode()).hexdigest()[:12]
    fat = os.path.join(tmp, tag + "_" + os.path.basename(obj) + ".fatbin")
    co = os.path.join(tmp, tag + "_" + os.path.basename(obj) + ".co")
    r = subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", obj, os.devnull], capture_output=True)
    if r.returncode != 0 or not os.path.exists(fat) or os.path.getsize(fat) == 0:
        return None
    subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                           f"--input={fat}", f"--output={co}"])
    return co if os.path.getsize(co) else None


def sha(path):
    return hashlib.sha256(open(path, "rb").read()).hexdigest()


def kernels(co):
    """{symbol: (instruction lines, descriptor lines)} of one code object"""
    syms = subprocess.check_output([f"{LLVM}/llvm-readelf", "-sW", co], text=True)
    kds = {m.group(1) for m in re.finditer(r"OBJECT\s+\w+\s+\w+\s+\d+\s+(\S+)\.kd\s*$", syms, re.M)}
    # without addresses and encodings a branch prints as its distance in dwords: the text does not depend on where the kernel lies
    dis = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", "-j", ".text", co], text=True)
    out, name = {}, None
    for line in dis.splitlines():
        m = re.match(r"^<(\S+)>:$", line)
        if m:
            name = m.group(1)
            assert name in kds, f"{co}: code under {name}, which is no kernel"
            out[name] = ([], [])
        elif name and line.startswith("\t") and line.strip() != "...":
            out[name][0].append(line.split("//")[0].strip())
    kd = subprocess.check_output([f"{LLVM}/llvm-objdump", "-d", "-j", ".rodata", co], text=True)
    name = None
    for line in kd.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)\.kd>:$", line)
        if m:
            name = m.group(1)
        elif name in out and line.startswith("\t.amdhsa_"):
            out[name][1].append(line.strip())
    assert set(out) == kds and all(d for _, d in out.values()), f"{co}: kernels without code or descriptor"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent"); ap.add_argument("change")
    ap.add_argument("--moved", default="")
    ap.add_argument("--rename", action="append", default=[])
    ap.add_argument("--out")
    a = ap.parse_args()
    old_name, new_names = (a.moved.split("=")[0], a.moved.split("=")[1].split(",")) if a.moved else (None, [])
    lines, bad = [], 0
    with tempfile.TemporaryDirectory() as tmp:
        names = lambda d: sorted(f[:-2] for f in os.listdir(d) if f.endswith(".o"))
        lines.append("# code objects of the other files: sha256 of the gfx950 code object, parent against change")
        for n in names(a.parent):
            if n == old_name:
                continue
            po, co_path = code_object(os.path.join(a.parent, n + ".o"), tmp), os.path.join(a.change, n + ".o")
            co = code_object(co_path, tmp) if os.path.exists(co_path) else None
            if po is None and co is None:
                lines.append(f"{n}.o  no device code on either side")
                continue
            same = po and co and sha(po) == sha(co)
            bad += not same
            lines.append(f"{n}.o  {sha(po)[:16] if po else '-'}  {sha(co)[:16] if co else '-'}  {'identical' if same else 'DIFFERENT'}")
        extra = [n for n in names(a.change) if n not in names(a.parent) and n not in new_names]
        bad += len(extra)
        lines += [f"{n}.o  only in the change" for n in extra]
        old = kernels(code_object(os.path.join(a.parent, old_name + ".o"), tmp)) if old_name else {}
        for r in a.rename:
            pat, repl = r.split("=", 1)
            old = {re.sub(pat, repl, k): v for k, v in old.items()}
        new, where = {}, {}
        for n in new_names:
            for k, v in kernels(code_object(os.path.join(a.change, n + ".o"), tmp)).items():
                new[k], where[k] = v, n
        if old_name:
            lines.append(f"# kernels of {old_name}.o ({len(old)}) against {', '.join(x + '.o' for x in new_names)} ({len(new)}): "
                         "symbol, file, instructions, instruction text and resource record identical")
        for k in sorted(set(old) | set(new)):
            if k not in old or k not in new:
                bad += 1
                lines.append(f"{k}  {'only in the parent' if k in old else 'only in the change (' + where[k] + '.o)'}")
                continue
            same = old[k] == new[k]
            bad += not same
            lines.append(f"{k}  {where[k]}.o  {len(new[k][0])}  {'yes' if same else 'NO'}")
            if not same:
                import difflib
                # the resource record first and whole (a cut-off instruction diff must not hide it), then the instructions, cut at 60 lines
                rec = [d for d in difflib.unified_diff(old[k][1], new[k][1], "parent", "change", lineterm="", n=0) if d[:1] in "+-" and d[:3] not in ("+++", "---")]
                lines.append(f"    resource record: {'identical' if not rec else 'DIFFERENT'}; instructions: {len(old[k][0])} -> {len(new[k][0])}")
                lines += ["    " + d for d in rec]
                for d in list(difflib.unified_diff(old[k][0], new[k][0], "parent", "change", lineterm="", n=1))[:60]:
                    lines.append("    " + d)
        lines.append(f"# {'all identical' if not bad else str(bad) + ' DIFFERENT'}")
    text = "\n".join(lines) + "\n"
    if a.out:
        open(a.out, "w").write(text)
    sys.stdout.write(text if bad or not a.out else "\n".join(l for l in lines if l.startswith("#")) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
