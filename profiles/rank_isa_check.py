"""Offline check that the existing phase-1 instantiations are unchanged by the ranking PAIR parameter.

Compile fm_batch_kernels.hip of both trees with the build's flags plus --save-temps, then
    python profiles/rank_isa_check.py <before>/fm_batch_kernels-hip-amdgcn-amd-amdhsa-gfx950.s <after>/fm_batch_kernels-hip-amdgcn-amd-amdhsa-gfx950.s
Every fm_rows_forward_k<T, LPR, TRAIN, WGT, SPLIT> of <before> is compared with fm_rows_forward_k<..., PAIR = false> of <after>, instruction
by instruction; assembler comments, local label numbers and the kernel's own name are ignored."""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from isa_check import funcs  # noqa: E402


def main(before, after):
    a, b = funcs(before), funcs(after)
    rows = [n for n in a if 'fm_rows_forward_k' in n]
    same = 0
    for n in rows:
        m = re.match(r'(_ZN3fmx17fm_rows_forward_kI.*?)(EEvNS_8RowsArgsENS_5HyperE)$', n)
        nn = m.group(1) + 'Lb0E' + m.group(2)
        if b.get(nn) == a[n]:
            same += 1
        else:
            print('differs or missing:', n)
    new = sum(1 for n in b if re.search(r'fm_rows_forward_k.*Lb1EEEvNS_8RowsArgs', n))
    print(f'fm_rows_forward_k instantiations before: {len(rows)}, identical after: {same}; PAIR instantiations: {new}')
    return 0 if same == len(rows) else 1


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
