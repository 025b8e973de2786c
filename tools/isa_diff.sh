#!/bin/bash
# Whether two trees compile the same device code: the gfx950 assembly of each given .hip source (paths below
# l3ac_amd/csrc), built with build.py's flags and PER_FILE_FLAGS of the second tree, compared as whole text, e.g.
#   tools/isa_diff.sh ../parent . kernels/gemm_split.hip kernels/attention.hip
# Lines that differ between two compiles of one unchanged file (the random __hip_cuid_ symbol, .file, .ident) are dropped.
# Prints one line per file and exits 1 if any differs.  ISA_DIFF_JOBS (default 4) files are compiled at a time; ISA_DIFF_KEEP=<dir>
# keeps the two texts of every file that differs there.
set -e
[ $# -ge 3 ] || { echo "usage: $0 TREE_A TREE_B FILE.hip..." >&2; exit 2; }
A="$(cd "$1" && pwd)"; B="$(cd "$2" && pwd)"; shift 2
OUT="$(mktemp -d)"
trap 'rm -rf "$OUT"' EXIT

per_file_flags() {  # PER_FILE_FLAGS[$1] of tree B's build.py (which imports the standard library only)
    python3 - "$B/l3ac_amd/build.py" "$1" <<'EOF'
import importlib.util, sys
spec = importlib.util.spec_from_file_location("l3ac_build", sys.argv[1])
mod = importlib.util.module_from_spec(spec)
spec.loader.exec_module(mod)
print(" ".join(mod.PER_FILE_FLAGS.get(sys.argv[2], [])))
EOF
}

isa() {  # tree, source, output
    /opt/rocm/bin/hipcc -O3 -std=c++17 --offload-arch=gfx950 -fPIC -Wall -Wno-unused-function -I"$1/include" -I"$1/l3ac_amd/csrc" \
        $(per_file_flags "$2") --cuda-device-only -S "$1/l3ac_amd/csrc/$2" -o "$3.raw" 2> "$3.err" || { cat "$3.err" >&2; return 1; }
    grep -v -e '__hip_cuid_' -e '^[[:space:]]*\.file' -e '^[[:space:]]*\.ident' "$3.raw" > "$3"
}

one() {
    local name="${1//\//_}"
    isa "$A" "$1" "$OUT/a_$name.s" && isa "$B" "$1" "$OUT/b_$name.s" || { echo "$1: FAILED TO COMPILE"; return 1; }
    if cmp -s "$OUT/a_$name.s" "$OUT/b_$name.s"; then
        echo "$1: identical ($(wc -l < "$OUT/b_$name.s") lines)"
    else
        echo "$1: DIFFERENT ($(diff "$OUT/a_$name.s" "$OUT/b_$name.s" | grep -c '^[<>]') lines)"
        [ -z "$ISA_DIFF_KEEP" ] || { mkdir -p "$ISA_DIFF_KEEP" && cp "$OUT/a_$name.s" "$OUT/b_$name.s" "$ISA_DIFF_KEEP/"; }
        return 1
    fi
}

export -f per_file_flags isa one
export A B OUT ISA_DIFF_KEEP
printf '%s\n' "$@" | xargs -P "${ISA_DIFF_JOBS:-4}" -I{} bash -c 'one "$1"' _ {} | sort > "$OUT/report"
cat "$OUT/report"
! grep -q -v ': identical' "$OUT/report"
