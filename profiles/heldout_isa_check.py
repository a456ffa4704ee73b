"""Offline check that sharing fm_topk.hip's pieces with fm_heldout.hip leaves every top-K kernel unchanged.

Compile fm_topk.hip of both trees with the build's flags plus --save-temps, then
    python profiles/heldout_isa_check.py <before>/fm_topk-hip-amdgcn-amd-amdhsa-gfx950.s <after>/fm_topk-hip-amdgcn-amd-amdhsa-gfx950.s
Every device function of <before> is compared with the function of the same name in <after>, instruction by instruction, and so are the
kernels' resource records (.vgpr_count, .sgpr_count, LDS, scratch); assembler comments, local label numbers and the kernel's own name are
ignored."""
import re
import sys


def funcs(path):
    s = open(path).read()
    out = {}
    for m in re.finditer(r'^(_Z\S+):', s, re.M):
        name = m.group(1)
        end = s.find('.Lfunc_end', m.end())
        body = s[m.end():end]
        body = re.sub(r'\.L\w+', 'L', body)
        body = '\n'.join(line.split(';')[0].rstrip() for line in body.splitlines())
        body = body.replace(name, 'KERNEL')
        out[name] = '\n'.join(line for line in body.splitlines() if line.strip())
    return out


def resources(path):
    """the metadata record of every kernel (amdhsa.kernels): its register counts, LDS, scratch and spills"""
    s = open(path).read()
    meta = s[s.find('amdhsa.kernels:'):]
    out = {}
    for rec in re.split(r'\n\s+- \.(?=agpr_count|args)', meta)[1:]:
        m = re.search(r'\.name:\s+(_Z\S+)', rec)
        if m:
            out[m.group(1)] = sorted(re.findall(r'\.(vgpr_count|sgpr_count|agpr_count|group_segment_fixed_size|private_segment_fixed_size|'
                                                r'vgpr_spill_count|sgpr_spill_count):\s+(\d+)', rec))
    return out


def main(before, after):
    a, b = funcs(before), funcs(after)
    same = sum(1 for n in a if b.get(n) == a[n])
    for n in a:
        if b.get(n) != a[n]:
            print('differs or missing:', n)
    ra, rb = resources(before), resources(after)
    rsame = sum(1 for n in ra if rb.get(n) == ra[n])
    print(f'fm_topk.hip functions before: {len(a)}, identical after: {same}; after holds {len(b)}; resource records identical: {rsame} of {len(ra)}')
    return 0 if same == len(a) and len(b) == len(a) and rsame == len(ra) else 1


if __name__ == '__main__':
    sys.exit(main(sys.argv[1], sys.argv[2]))
