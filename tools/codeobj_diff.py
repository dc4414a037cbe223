#!/usr/bin/env python3
"""Compares the kernels of two sets of gfx950 device code objects (host only):
  codeobj_diff.py --a parent/*.co --b branch/*.co
A code object comes out of a HIP object file with
  llvm-objcopy -O binary --only-section=.hip_fatbin x.o x.hipfb
  clang-offload-bundler --unbundle --type=o --input=x.hipfb --output=x.co \\
      --targets=hipv4-amdgcn-amd-amdhsa--gfx950
For every kernel in both sets: the resource metadata of its note, then its
instructions and those of the out-of-line functions it calls, without addresses
and padding.  PC-relative immediates of s_getpc sequences differ once code
moves: they become the name of the function or object they point at, or <pcrel>
where no symbol starts there (constants in .rodata: a kernel that read other
constants would still compare equal).  LLVM_BIN: the tools' folder.
"""
import argparse, difflib, os, re, subprocess

LLVM = os.environ.get('LLVM_BIN', '/opt/rocm/llvm/bin')
META = ('.vgpr_count', '.sgpr_count', '.agpr_count', '.group_segment_fixed_size', '.private_segment_fixed_size',
        '.vgpr_spill_count', '.sgpr_spill_count', '.kernarg_segment_size', '.max_flat_workgroup_size')
run = lambda tool, *args: subprocess.check_output([os.path.join(LLVM, tool), *args], text=True)


def load(path):
    """{kernel: (metadata, instructions of the kernel and its callees)} of one code object."""
    meta = {}
    for block in re.split(r'\n  - (?=\.)', run('llvm-readelf', '--notes', path))[1:]:
        kv = dict(re.findall(r'^(?:    )?(\.\w+): +(\S+)$', block, re.M))
        meta[kv['.name']] = {k: kv.get(k) for k in META}
    sym_at = {}  # address -> (name, is a function)
    for m in re.finditer(r'^ *\d+: ([0-9a-f]+) +\d+ (FUNC|OBJECT) .* (\S+)$', run('llvm-readelf', '-sW', path), re.M):
        sym_at[int(m.group(1), 16)] = (m.group(3), m.group(2) == 'FUNC')
    body, calls, cur, pc = {}, {}, None, {}
    for line in run('llvm-objdump', '-d', path).splitlines():
        m = re.match(r'^[0-9a-f]+ <(.+)>:$', line)
        if m:
            cur, pc = m.group(1), {}
            body[cur], calls[cur] = [], []
        elif cur is not None and line.startswith('\t') and '//' in line:
            text, addr = line.split('//')[0].split(), int(line.split('//')[1].split(':')[0], 16)
            if text[0] == 's_getpc_b64':
                pc[re.match(r's\[(\d+):', text[1]).group(1)] = addr + 4
            elif text[0] == 's_add_u32' and text[1] == text[2] and text[1][1:-1] in pc:
                reg, imm = text[1][1:-1], int(text[3], 0)
                name, is_func = sym_at.get(pc.pop(reg) + (imm - (1 << 32) if imm >= 1 << 31 else imm), ('pcrel', False))
                pc['hi' + str(int(reg) + 1)] = True
                text[3] = '<%s>' % name
                if is_func:
                    calls[cur].append(name)
            elif text[0] == 's_addc_u32' and text[1] == text[2] and pc.pop('hi' + text[1][1:-1], False):
                text[3] = '<pcrel-hi>'
            body[cur].append(' '.join(text))
    out = {}
    for k in meta:
        seen, todo, ins = [], [k], []
        while todo:
            f = todo.pop(0)
            if f not in seen:
                seen.append(f)
                code = body[f][:]
                while code and code[-1] == 's_nop 0':  # the padding up to the next function
                    code.pop()
                ins += ['<%s>:' % f] + code
                todo += calls[f]
        out[k] = (meta[k], ins)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--a', nargs='+', required=True)
    ap.add_argument('--b', nargs='+', required=True)
    args = ap.parse_args()
    A, B, twice = {}, {}, []
    for kernels, paths in ((A, args.a), (B, args.b)):
        for k, v in [kv for p in paths for kv in load(p).items()]:
            twice += [k] if k in kernels else []
            kernels[k] = v
    n_meta = n_code = 0
    for k in sorted(A.keys() & B.keys()):
        (ma, ia), (mb, ib) = A[k], B[k]
        diff = ['%s %s -> %s' % (key, ma[key], mb[key]) for key in META if ma[key] != mb[key]]
        n_meta += bool(diff)
        if ia != ib:
            n_code += 1
            lines = sum(d[0] in '+-' for d in difflib.unified_diff(ia, ib, lineterm='', n=0)) - 2
            diff.append('instructions differ: %d vs %d, %d lines of diff' % (len(ia), len(ib), lines))
        print('%-90s %s' % (k, '; '.join(diff) or 'identical'))
    for k in sorted(A.keys() ^ B.keys()) + twice:
        print('%s: %s' % ('twice in one set' if k in twice else 'only in a' if k in A else 'only in b', k))
    print('summary: %d kernels in a, %d in b, %d in both: %d with metadata differences, %d with instruction '
          'differences; %d on one side only, %d defined twice' %
          (len(A), len(B), len(A.keys() & B.keys()), n_meta, n_code, len(A.keys() ^ B.keys()), len(twice)))


main()
