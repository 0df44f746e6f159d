"""Is the device code of two builds of one HIP source the same?  Compares, kernel by kernel, the instruction text and kernel descriptor of two
device-only assembly files and the figures of their -Rpass-analysis=kernel-resource-usage reports; the order of the kernels in the file may
differ.  Both sides are compiled from the same path (or with one fixed -cuid=) so that symbols of internal linkage carry the same name:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 <DEFAULT_FLAGS of build.py> --cuda-device-only -S -cuid=x \
          -Rpass-analysis=kernel-resource-usage FILE.hip -o SIDE.s 2> SIDE.remarks
    python tools/device_identity.py parent.s parent.remarks new.s new.remarks

Prints the verdict and one table row per kernel; exit status 1 on any difference."""
import re
import sys

FIGURES = ('TotalSGPRs', 'VGPRs', 'AGPRs', 'ScratchSize [bytes/lane]', 'LDS Size [bytes/block]', 'Occupancy [waves/SIMD]')


def kernels(asm):
    """symbol -> (instruction text, descriptor text); local labels lose the function's index in the file (.LBB12_3 -> .LBB_3)"""
    text = re.sub(r'\.L(BB|func_begin|func_end|tmp)\d+', r'.L\1', open(asm).read())
    text = re.sub(r'\bBB\d+_', 'BB_', text)                    # (the same index in the loop comments ...
    text = re.sub(r'[ \t]+;', ' ;', text)                      #  ... whose column moves with the number of its digits)
    out = {}
    for m in re.finditer(r'^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel', text, re.S | re.M):
        sym = m.group(1)
        body = re.search(r'^%s:[^\n]*\n(.*?)^\.Lfunc_end' % re.escape(sym), text, re.S | re.M).group(1)
        out[sym] = (body, m.group(2))
    return out


def usage(remarks):
    out, cur = {}, None
    for line in open(remarks):
        m = re.search(r'remark:\s+(.*?): (\S+) \[-Rpass-analysis', line)
        if not m:
            continue
        if m.group(1) == 'Function Name':
            cur = out.setdefault(m.group(2), {})
        elif cur is not None and m.group(1) in FIGURES:
            cur[m.group(1)] = m.group(2)
    return out


def main(pa, pr, na, nr):
    ka, kb, ua, ub = kernels(pa), kernels(na), usage(pr), usage(nr)
    bad = []
    if set(ka) != set(kb):
        bad.append(f'kernel symbols differ: only parent {sorted(set(ka) - set(kb))}, only new {sorted(set(kb) - set(ka))}')
    rows = []
    for sym in sorted(set(ka) & set(kb)):
        same_text, same_desc, same_use = ka[sym][0] == kb[sym][0], ka[sym][1] == kb[sym][1], ua.get(sym) == ub.get(sym) and sym in ua
        if not (same_text and same_desc and same_use):
            bad.append(f'{sym}: instructions {"equal" if same_text else "DIFFER"}, descriptor {"equal" if same_desc else "DIFFER"}, '
                       f'resource usage {"equal" if same_use else "DIFFER"}')
        insts = sum(1 for l in ka[sym][0].split('\n') if l.startswith('\t') and not l.startswith('\t.') and not l.startswith('\t;'))
        rows.append((sym, insts, ua.get(sym, {}), ub.get(sym, {}), same_text and same_desc))
    print(f'{len(ka)} kernels in the parent, {len(kb)} in the new build; ' + ('IDENTICAL: same symbols, same instruction text, same descriptors, '
          'same resource usage' if not bad else f'{len(bad)} DIFFERENCES'))
    for b in bad:
        print('  ' + b)
    print('\nper kernel: instructions, then parent / new of SGPRs, VGPRs, AGPRs, scratch bytes per lane, static LDS bytes, occupancy; text = instruction text and descriptor')
    for sym, insts, a, b, same in rows:
        print(f'{sym}\n    {insts:6d} instr   ' + '   '.join(f'{a.get(f, "?")}/{b.get(f, "?")}' for f in FIGURES) + f'   text {"equal" if same else "DIFFERS"}')
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main(*sys.argv[1:5]))
