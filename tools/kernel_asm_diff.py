"""Compare the device code of two builds kernel by kernel (no GPU needed): for a change that must leave kernels as they are.

    cd m3vit_amd/csrc
    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S -fuse-cuid=none wgrad_dma.hip -o new_dma.s    # per source
    python tools/kernel_asm_diff.py old_wgrad.s -- new_wgrad.s new_staged.s new_dma.s

Either side may be several files (a source that was split).  Per mangled kernel name the text from the kernel's label to
its end is compared - instructions and the .amdhsa_ kernel descriptor - with comments dropped and the local labels, which
carry the function's number in its file (.LBB12_3, .Lfunc_end12), renumbered.  Prints the kernels that are missing, new or
different and exits 1 if there are any."""
import re
import sys


def _norm(line):
    line = line.split(';')[0].rstrip()
    line = re.sub(r'\.LBB\d+_', '.LBB_', line)
    return re.sub(r'\.Lfunc_(end|begin)\d+', r'.Lfunc_\1', line)


def kernels(paths):
    out = {}
    for path in paths:
        lines = open(path).read().split('\n')
        i = 0
        while i < len(lines):
            m = re.match(r'\s*\.type\s+(\S+),@function', lines[i])
            if m:
                j = i
                while not re.match(r'\.Lfunc_end\d+:', lines[j]):
                    j += 1
                assert m.group(1) not in out, f'{m.group(1)} defined twice'
                out[m.group(1)] = [x for x in map(_norm, lines[i:j]) if x.strip()]
                i = j
            i += 1
    return out


def main():
    k = sys.argv.index('--')
    old, new = kernels(sys.argv[1:k]), kernels(sys.argv[k + 1:])
    both = sorted(set(old) & set(new))
    differ = [n for n in both if old[n] != new[n]]
    print(f'{len(old)} kernels before, {len(new)} after; missing {sorted(set(old) - set(new))}, new {sorted(set(new) - set(old))}')
    for n in differ:
        lines = sum(1 for a, b in zip(old[n], new[n]) if a != b) if len(old[n]) == len(new[n]) else None
        print(f'DIFFERENT {n}: {len(old[n])} -> {len(new[n])} lines' + (f', {lines} of them changed in place' if lines is not None else ''))
    print(f'compared {len(both)}, different {len(differ)}')
    return 1 if differ or set(old) != set(new) else 0


if __name__ == '__main__':
    sys.exit(main())
