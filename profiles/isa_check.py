"""Offline check that a change leaves the compiled kernels as they were: two assembly files are compared function by function.

Compile the touched .hip files of both trees with the build's flags (fmwr_amd/build.py) plus --save-temps, then
    python profiles/isa_check.py [--gone REGEX] [--new REGEX] [--rename OLD_REGEX=NEW ...] [--ignore-kernarg-layout] <before>/fm_topk-hip-amdgcn-amd-amdhsa-gfx950.s <after>/fm_topk-hip-amdgcn-amd-amdhsa-gfx950.s \
                                                              <before>/fm_pairs-hip-amdgcn-amd-amdhsa-gfx950.s <after>/fm_pairs-hip-amdgcn-amd-amdhsa-gfx950.s ...
Every function of <before> is compared with the function of the same name in <after>, instruction by instruction, and so are the kernels'
resource records (.vgpr_count, .sgpr_count, LDS, scratch, spills); assembler comments, local label numbers and the function's own name are
ignored, and symbols that are data rather than code (no function end before the next symbol) are left out.  A function of <before> may be
missing from <after> only if its name matches --gone.  A function that only <after> holds must match --new; it is listed with its resource
record and must not spill or use scratch.  The exit status is 0 only if every pair passes.
--rename OLD_REGEX=NEW (repeatable; re.sub on the names of <before>) pairs a function whose mangled name changed -- a template parameter that went -- with its
successor.  --ignore-kernarg-layout masks the offset immediate of every s_load_* and skips .amdhsa_kernarg_size: a kernel-argument struct that lost fields
moves every later field.  A pair that differs is listed with its instruction counts and both resource records."""
import argparse
import re
import sys

SPILLS = ('vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size')


def funcs(path, ignore_kernarg=False):
    """name -> normalised body of every function (_Z symbol that ends in a .Lfunc_end before the next symbol)"""
    s = open(path).read()
    heads = list(re.finditer(r'^(_Z\S+):', s, re.M))
    out = {}
    for i, m in enumerate(heads):
        name = m.group(1)
        end = s.find('.Lfunc_end', m.end())
        if end < 0 or (i + 1 < len(heads) and end > heads[i + 1].start()):
            continue
        body = s[m.end():end]
        body = re.sub(r'\.L\w+', 'L', body)
        body = '\n'.join(line.split(';')[0].rstrip() for line in body.splitlines())
        body = body.replace(name, 'KERNEL')
        if ignore_kernarg:
            body = re.sub(r'^([ \t]*s_load_\w+[ \t].*,[ \t]*)(0x[0-9a-fA-F]+|\d+)[ \t]*$', r'\1OFFSET', body, flags=re.M)
            body = re.sub(r'^\s*\.amdhsa_kernarg_size.*$', '', body, flags=re.M)
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


def renamed(d, renames):
    out = {}
    for n, v in d.items():
        for pat, to in renames:
            n = re.sub(pat, to, n)
        out[n] = v
    return out


def compare(before, after, gone, new, renames=(), ignore_kernarg=False):
    a, b = renamed(funcs(before, ignore_kernarg), renames), funcs(after, ignore_kernarg)
    ra, rb = renamed(resources(before), renames), resources(after)
    ok = True
    same = left = 0
    for n in a:
        if n not in b and gone and re.search(gone, n):
            left += 1
        elif b.get(n) == a[n]:
            same += 1
        else:
            print('differs' if n in b else 'missing', n)
            if n in b:
                print(f'       instructions {len(a[n].splitlines())} -> {len(b[n].splitlines())}')
                print('       before: ' + ', '.join(f'{k} {v}' for k, v in ra.get(n, [])))
                print('       after:  ' + ', '.join(f'{k} {v}' for k, v in rb.get(n, [])))
            ok = False
    rsame = rleft = 0
    for n in ra:
        if n not in rb and n not in b and gone and re.search(gone, n):
            rleft += 1
        elif rb.get(n) == ra[n]:
            rsame += 1
        else:
            print('resource record differs or missing', n)
            ok = False
    added = [n for n in b if n not in a]
    what = re.sub(r'-hip-amdgcn.*$', '', after.replace('\\', '/').rsplit('/', 1)[-1])
    print(f'{what}: functions before {len(a)}, identical after {same}, gone {left}; resource records identical {rsame} of {len(ra) - rleft}'
          f' (gone {rleft}); new functions {len(added)}')
    for n in added:
        rec = dict(rb.get(n, []))
        print(f'  new: {n}')
        if rec:
            print('       ' + ', '.join(f'{k} {v}' for k, v in sorted(rec.items())))
        if not (new and re.search(new, n)):
            print('       (not expected: no match of --new)')
            ok = False
        if any(int(rec.get(k, 0)) for k in SPILLS):
            print('       spills or scratch')
            ok = False
    return ok


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--gone', help='functions of <before> that may be missing from <after>')
    ap.add_argument('--new', help='functions that only <after> may hold')
    ap.add_argument('--rename', action='append', default=[], metavar='OLD_REGEX=NEW', help='re.sub applied to the function names of <before> (repeatable)')
    ap.add_argument('--ignore-kernarg-layout', action='store_true', help='mask s_load_* offsets and skip .amdhsa_kernarg_size')
    ap.add_argument('files', nargs='+', help='before.s after.s [before.s after.s ...]')
    args = ap.parse_args(argv)
    if len(args.files) % 2:
        ap.error('the assembly files come in pairs: before.s after.s')
    renames = [tuple(r.split('=', 1)) for r in args.rename]
    if any(len(r) != 2 for r in renames):
        ap.error('--rename takes OLD_REGEX=NEW')
    ok = True
    for i in range(0, len(args.files), 2):
        ok = compare(args.files[i], args.files[i + 1], args.gone, args.new, renames, args.ignore_kernarg_layout) and ok
    print('ISA check:', 'PASS' if ok else 'FAIL')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
