#!/usr/bin/env python3
"""Per-kernel digest of a build's gfx950 device code: the way to show that a move of kernel code between files (or any change meant to leave the
machine code alone) did so.  For every kernel of every object of BUILD_DIR: the mangled name, a sha256 over its instruction ENCODINGS (the hex
words after `// <addr>:` in `llvm-objdump -d`: not the text, whose `<label+off>` annotations and asm-statement label ids differ between
translation units) and the metadata that decides occupancy and launch (register counts, spills, LDS, scratch, kernarg size).  Two builds hold
the same device code when the sorted tables are equal (`diff`); the object a kernel sits in is not part of its line.
usage: kernel_digest.py BUILD_DIR            (devit_amd/csrc/build after build.sh)"""
import glob
import hashlib
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "devit_amd", "csrc"))
import check_objects as CO  # noqa: E402

FIELDS = (".sgpr_count", ".vgpr_count", ".agpr_count", ".vgpr_spill_count", ".sgpr_spill_count", ".group_segment_fixed_size",
          ".private_segment_fixed_size", ".kernarg_segment_size", ".max_flat_workgroup_size")


def encodings(disassembly):
    """kernel symbol -> (sha256 over its instruction words in order, number of words) from `llvm-objdump -d` text; the `<L_...>` labels of asm
    statements stay inside their kernel; EVERY instruction line counts, one whose encoding cannot be read ends the run (tests/test_abi.py feeds it
    synthetic text)"""
    h, cur = {}, None
    for line in disassembly.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            if not m.group(1).startswith("L_"):
                cur = m.group(1)
                h[cur] = [hashlib.sha256(), 0]
            continue
        if cur is None or not re.search(r"//\s*[0-9A-Fa-f]+:", line):
            continue
        # (a branch carries its target as `<label+off>` behind the words: that annotation is skipped, the words are not)
        m = re.search(r"//\s*[0-9A-Fa-f]+:((?:\s+[0-9A-Fa-f]{8})+)\s*(?:<[^>]*>)?\s*$", line)
        if not m:
            sys.exit(f"kernel_digest: {cur}: cannot read the encoding of `{line.strip()[:120]}`: no instruction may be left out")
        words = m.group(1).split()
        h[cur][0].update((" ".join(words) + "\n").encode())
        h[cur][1] += len(words)
    return {k: (v[0].hexdigest(), v[1]) for k, v in h.items()}


def metadata(notes):
    """kernel symbol -> {field: value} from `llvm-readelf --notes`: the entries of amdhsa.kernels start with `  - .key:`, their own keys sit at that
    depth (the keys of .args entries lie deeper and are skipped)"""
    kernels, ent = {}, None
    for line in notes.splitlines():
        m = re.match(r"^  (- |  )(\.\w+):\s*(\S*)\s*$", line)
        if not m:
            continue
        if m.group(1) == "- ":
            ent = {}
        if ent is None:
            continue
        ent[m.group(2)] = m.group(3)
        if m.group(2) == ".name":
            kernels[m.group(3)] = ent
    return kernels


def main(build):
    CO.tools_present()
    rows = []
    for obj in sorted(glob.glob(os.path.join(build, "*.o"))):
        f = os.path.basename(obj)[:-2]
        with CO.code_object(build, f) as co:
            if co is None:
                continue
            enc = encodings(CO.run(os.path.join(CO.LLVM, "llvm-objdump"), "-d", co))
            meta = metadata(CO.run(os.path.join(CO.LLVM, "llvm-readelf"), "--notes", co))
            if set(enc) != set(meta):
                sys.exit(f"kernel_digest: {f}.o: disassembly and metadata name different kernels: {sorted(set(enc) ^ set(meta))[:4]}")
            for k in enc:
                rows.append(f"{k} sha256={enc[k][0]} words={enc[k][1]} " + " ".join(f"{x[1:]}={meta[k].get(x, '-')}" for x in FIELDS))
    if not rows:
        sys.exit("kernel_digest: no kernel found")
    print("\n".join(sorted(rows)))
    print(f"# {len(rows)} kernels")


if __name__ == "__main__":
    main(sys.argv[1])
