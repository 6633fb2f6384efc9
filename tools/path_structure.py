#!/usr/bin/env python3
"""Control structure of the step of a kernel in a gfx950 assembly listing: on the cycle tools/main_path.py finds (cheapest, or forced through the
logging blocks with --logged), how many branch instructions are taken and how many fall through, the scalar-ALU opcodes by count, and the
instruction classes of tools/isa_stats.py.  Counts instruction classes only; the resource lines are the assembler's own metadata of the kernel.

usage: tools/path_structure.py listing.s [substring-of-kernel-name] [--logged | --through=REGEX] [--branches]"""
import collections
import re
import sys

import isa_stats
import main_path


def resources(listing, name):
    """vgpr / agpr / sgpr-spill / LDS / scratch figures from the kernel's metadata entry in the listing."""
    text = open(listing).read()
    at = text.find('.name:', text.find('amdhsa.kernels'))
    out = {}
    for entry in text[at:].split('  - .')[0:] if at >= 0 else []:
        if f'.name:           {name}' not in entry and f'.name: {name}' not in entry:
            continue
        for key in ('.vgpr_count', '.agpr_count', '.sgpr_count', '.sgpr_spill_count', '.vgpr_spill_count', '.group_segment_fixed_size', '.private_segment_fixed_size'):
            m = re.search(re.escape(key) + r':\s+(\d+)', entry)
            if m:
                out[key[1:]] = int(m.group(1))
        break
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith('--')]
    through = next((a.split('=', 1)[1] for a in sys.argv[1:] if a.startswith('--through=')), None)
    if '--logged' in sys.argv:
        through = main_path.LOGGED
    name, bl, path = main_path.step_path(args[0], args[1] if len(args) > 1 else None, through)
    taken = fall = 0
    kinds = collections.Counter()
    ins = []
    for pos, k in enumerate(path):
        ins += bl[k][1]
        nxt = path[(pos + 1) % len(path)]
        last = bl[k][1][-1].split() if bl[k][1] else ['']
        if last[0].startswith('s_cbranch') or last[0] == 's_branch':
            goes = last[0] == 's_branch' or not (nxt == k + 1 and bl[nxt][0] != last[1])
            taken, fall = taken + goes, fall + (not goes)
            kinds[last[0] + (' taken' if goes else ' not taken')] += 1
            if '--branches' in sys.argv:
                print(f'    {bl[k][0]:12s} {" ".join(last):34s} {"taken -> " + bl[nxt][0] if goes else "falls through"}')
    ops = [i.split()[0] for i in ins]
    salu = collections.Counter(o for o in ops if isa_stats.classify(o) == 'salu' and not o.startswith(('s_cbranch', 's_branch')))
    print(f'{name}\n  {"step through " + through if through else "cheapest step"}: {len(path)} blocks, {len(ops)} instructions')
    print(f'  branches: {taken} taken (the back edge included), {fall} not taken   ' + ', '.join(f'{k} {v}' for k, v in sorted(kinds.items())))
    print(f'  scalar ALU without branches: {sum(salu.values())}   ' + ', '.join(f'{k} {v}' for k, v in salu.most_common()))
    print('  classes: ' + ', '.join(f'{k} {v}' for k, v in collections.Counter(isa_stats.classify(o) for o in ops).most_common()))
    res = resources(args[0], name)
    if res:
        print('  resources: ' + ', '.join(f'{k} {v}' for k, v in res.items()))


if __name__ == '__main__':
    main()
