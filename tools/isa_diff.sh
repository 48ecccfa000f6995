#!/bin/bash
# tools/isa_diff.sh PARENT_REF [FILE...] — which kernels' machine code does the working tree change against PARENT_REF?  (CPU only: hipcc
# cross-compiles.)  PARENT_REF is checked out into a temporary `git worktree`; in both trees every csrc/*.hip (or only FILE..., names
# without directory; a name that one tree lacks is skipped there: kernels are matched by name, so they may move between files) goes through
#   hipcc <the Makefile's flags> --cuda-device-only -S -Rpass-analysis=kernel-resource-usage
# and per kernel the instruction stream (comments and directives dropped, labels renumbered in order of definition: a label's number
# depends on what else the file holds) and the compiler's account (registers, spills, scratch, LDS, occupancy) are compared.
# One line per kernel: `same`, `DIFFERENT (...)`, `only in PARENT_REF`, `only in the working tree`.  Exit status 1 if a kernel that
# both trees have differs; the two normalised streams of such a kernel stay under $ISA_DIFF_KEEP (default: a temporary directory that
# is named) for `diff`.  EXTRA="-D..." as for make.
#   tools/isa_diff.sh HEAD                                   after an edit that should not touch any kernel
#   tools/isa_diff.sh main bgzf_copy.hip bgzf_symbols.hip    what a performance change did change
set -euo pipefail
[ $# -ge 1 ] || { sed -n '2,14p' "$0"; exit 2; }
ref=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
tmp=$(mktemp -d)
keep=${ISA_DIFF_KEEP:-$tmp/differing}
cleanup() { git -C "$root" worktree remove --force "$tmp/parent" 2>/dev/null || true; [ -d "$keep" ] && [ "$keep" = "$tmp/differing" ] || rm -rf "$tmp"; }
trap cleanup EXIT
git -C "$root" worktree add --quiet --detach "$tmp/parent" "$ref"

compile_tree() {        # TREE OUTDIR FILE...
    local src=$1/trueconsense_amd/csrc out=$2 flags f; shift 2
    mkdir -p "$out"
    # the flags as the tree's own Makefile has them
    flags=$(printf 'isa-flags:\n\t@echo --offload-arch=$(ARCH) $(CXXFLAGS) $(EXTRA)\n' | make -s --no-print-directory -C "$src" -f Makefile -f - isa-flags EXTRA="${EXTRA:-}" | tail -n 1)
    if [ $# -eq 0 ]; then set -- $(cd "$src" && ls *.hip); fi
    for f in "$@"; do
        [ -f "$src/$f" ] || continue
        ( cd "$src" && ${HIPCC:-hipcc} $flags --cuda-device-only -S -Rpass-analysis=kernel-resource-usage "$f" -o "$out/${f%.hip}.s" 2> "$out/${f%.hip}.remarks" ) \
            || { echo "isa_diff: $f of $1 does not compile:" >&2; grep -v 'remark:' "$out/${f%.hip}.remarks" >&2; exit 3; } &
    done
    wait
    for f in "$@"; do [ ! -f "$src/$f" ] || [ -s "$out/${f%.hip}.s" ] || exit 3; done
}
compile_tree "$tmp/parent" "$tmp/a" "$@"
compile_tree "$root" "$tmp/b" "$@"

python3 - "$tmp/a" "$tmp/b" "$ref" "$keep" <<'EOF'
import glob, os, re, subprocess, sys
dir_a, dir_b, ref, keep = sys.argv[1:5]

def kernels(d):
    """{mangled name: (normalised instruction stream, {resource: value})}"""
    out = {}
    for path in sorted(glob.glob(os.path.join(d, "*.s"))):
        lines = open(path).read().split("\n")
        names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
        for name in names:
            i = next(k for k, l in enumerate(lines) if l.startswith(name + ":"))
            body = []
            for l in lines[i + 1:]:
                if re.match(r"\.Lfunc_end\d+:", l): break
                l = l.split(";")[0].rstrip()                    # (no string operands in device code: a ';' starts a comment)
                if not l.strip() or l.strip().startswith("."):  # directives (.p2align, .loc ...); local labels start in column 0
                    if not re.match(r"[.\w$]+:", l): continue
                body.append(l.strip())
            labels = {}
            for l in body:
                m = re.match(r"([.\w$]+):$", l)
                if m: labels[m.group(1)] = "L%d" % len(labels)
            if labels:
                pat = re.compile(r"(?<![\w.$])(" + "|".join(sorted(map(re.escape, labels), key=len, reverse=True)) + r")(?![\w$])")
                body = [pat.sub(lambda m: labels[m.group(1)], l) for l in body]
            out[name] = ["\n".join(body) + "\n", {}]
        cur = None
        for l in open(path[:-2] + ".remarks"):
            m = re.search(r"remark:\s+(.*?)\s+\[-Rpass-analysis=kernel-resource-usage\]", l)
            if not m: continue
            key, _, val = m.group(1).partition(": ")
            if key == "Function Name": cur = out.get(val)
            elif cur is not None: cur[1][key.strip()] = val.strip()
    return out

def short(name):            # bgzf_copy<true,false>, as rocprofv3 prints it
    d = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip() or name
    d = re.sub(r"^void ", "", d).replace("(anonymous namespace)::", "")
    depth = 0
    for k, ch in enumerate(d):                                  # cut the argument list
        depth += ch == "<"; depth -= ch == ">"
        if ch == "(" and depth == 0: d = d[:k]; break
    return d.replace(", ", ",")

a, b = kernels(dir_a), kernels(dir_b)
bad = 0
for name in sorted(set(a) | set(b), key=short):
    if name not in b: print("%-44s only in %s" % (short(name), ref)); continue
    if name not in a: print("%-44s only in the working tree" % short(name)); continue
    (sa, ra), (sb, rb) = a[name], b[name]
    why = []
    if sa != sb: why.append("instructions: %d -> %d lines" % (sa.count("\n"), sb.count("\n")))
    why += ["%s: %s -> %s" % (k, ra.get(k), rb.get(k)) for k in sorted(set(ra) | set(rb)) if ra.get(k) != rb.get(k)]
    res = "VGPRs %s, SGPRs %s, spills %s + %s, scratch %s, LDS %s, occupancy %s" % tuple(rb.get(k, "?") for k in (
        "VGPRs", "TotalSGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]"))
    if why:
        bad += 1
        os.makedirs(keep, exist_ok=True)
        stem = os.path.join(keep, re.sub(r"\W+", "_", short(name)))
        open(stem + ".parent.s", "w").write(sa); open(stem + ".new.s", "w").write(sb)
        print("%-44s DIFFERENT (%s)" % (short(name), "; ".join(why)))
    else:
        print("%-44s same: %d instruction lines; %s" % (short(name), sb.count("\n"), res))
if bad: print("isa_diff: %d kernel(s) differ; their streams: %s" % (bad, keep))
sys.exit(1 if bad else 0)
EOF
