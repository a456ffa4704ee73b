"""Offline check that the hard-negative pass (fmx_matrix_pairs_hard) leaves the existing kernels unchanged.

Compile fm_pairs.hip and fm_topk.hip of both trees with the build's flags plus --save-temps, then
    python profiles/hardneg_isa_check.py <before>/fm_pairs-hip-amdgcn-amd-amdhsa-gfx950.s <after>/fm_pairs-hip-amdgcn-amd-amdhsa-gfx950.s \
                                         <before>/fm_topk-hip-amdgcn-amd-amdhsa-gfx950.s <after>/fm_topk-hip-amdgcn-amd-amdhsa-gfx950.s
Every function of <before> is compared with the function of the same name in <after>, instruction by instruction, and so are the kernels'
resource records (heldout_isa_check.py's rules).  Symbols that are data rather than code (no function end) are left out.  The functions that
only <after> holds are listed with their resource records: they must be the hard pass's kernels alone, without spills or scratch."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from heldout_isa_check import resources  # noqa: E402


def funcs(path):
    s = open(path).read()
    out = {}
    for m in re.finditer(r'^(_Z\S+):', s, re.M):
        name = m.group(1)
        end = s.find('.Lfunc_end', m.end())
        if end < 0:
            continue
        body = s[m.end():end]
        body = re.sub(r'\.L\w+', 'L', body)
        body = '\n'.join(line.split(';')[0].rstrip() for line in body.splitlines())
        body = body.replace(name, 'KERNEL')
        out[name] = '\n'.join(line for line in body.splitlines() if line.strip())
    return out


def compare(what, before, after, allowed_new):
    a, b = funcs(before), funcs(after)
    ra, rb = resources(before), resources(after)
    same = sum(1 for n in a if b.get(n) == a[n])
    for n in a:
        if b.get(n) != a[n]:
            print('differs or missing:', n)
    rsame = sum(1 for n in ra if rb.get(n) == ra[n])
    new = [n for n in b if n not in a]
    print(f'{what}: functions before {len(a)}, identical after {same}; resource records identical {rsame} of {len(ra)}; new functions {len(new)}')
    ok = same == len(a) and rsame == len(ra)
    for n in new:
        rec = dict(rb.get(n, []))
        print(f'  new: {n}')
        print('       ' + ', '.join(f'{k} {v}' for k, v in sorted(rec.items())))
        if not re.search(allowed_new, n):
            print('       (not a hard-pass kernel)')
            ok = False
        if any(int(rec.get(k, 0)) for k in ('vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size')):
            print('       spills or scratch')
            ok = False
    return ok


def main(pairs_before, pairs_after, topk_before, topk_after):
    ok = compare('fm_pairs.hip', pairs_before, pairs_after, r'hard_choose_k')
    ok = compare('fm_topk.hip', topk_before, topk_after, r'^$') and ok
    print('ISA check:', 'PASS' if ok else 'FAIL')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:5]))
