"""Static instruction counts and kernel metadata of agent-kernel instantiations in a device-only assembly listing of
csrc/die_pic.hip (hipcc <build.py's FLAGS> --cuda-device-only -S): profiles/r08_k1_specialised_isa.txt.

    python scratch/k1_isa_counts.py LISTING.s SYMBOL_PREFIX [SYMBOL_PREFIX ...]
    python scratch/k1_isa_counts.py --body-hash LISTING.s        (every k_pic_forward_move: sha1 of the body with the kernel's own symbol blanked)
"""
import hashlib
import re
import sys


def kernels(path):
    """{symbol: [instruction lines]} of every k_pic_forward_move instantiation, and the metadata entries by symbol."""
    bodies, cur = {}, None
    meta, mcur = {}, None
    for line in open(path):
        s = line.strip()
        m = re.match(r'^(_Z\d+k_pic_forward_move\w+):', s)
        if m:
            cur = m.group(1)
            bodies[cur] = []
            continue
        if cur is not None:
            if s.startswith('.Lfunc_end'):
                cur = None
            elif s and not s.startswith(('.', ';', '//')) and not s.endswith(':'):
                bodies[cur].append(s.split(';')[0].split('//')[0].strip())
        if s.startswith('- .agpr_count') or s.startswith('- .args'):
            mcur = {}
        m = re.match(r'^-?\s*\.(\w+):\s+(.*)$', s)
        if m and mcur is not None:
            k, v = m.group(1), m.group(2)
            if k in ('sgpr_count', 'sgpr_spill_count', 'vgpr_count', 'vgpr_spill_count', 'agpr_count', 'group_segment_fixed_size', 'private_segment_fixed_size', 'kernarg_segment_size', 'max_flat_workgroup_size', 'wavefront_size'):
                mcur[k] = v
            if k == 'symbol':
                meta[v.strip("'\"").replace('.kd', '')] = mcur
    return bodies, meta


def classify(ins):
    op = ins.split()[0]
    if op in ('v_readlane_b32', 'v_writelane_b32'):
        return 'lane'
    if op == 's_waitcnt':
        return 's_waitcnt'
    if op == 's_nop':
        return 's_nop'
    if op.startswith(('s_load_', 's_buffer_load_')):
        return 'sload'
    if op.startswith('v_'):
        return 'valu'
    if op.startswith('s_'):
        return 'salu'
    if op.startswith('ds_'):
        return 'lds'
    if op.startswith(('global_', 'flat_', 'buffer_', 'scratch_')):
        return 'vmem'
    return 'other'


def main():
    if sys.argv[1] == '--body-hash':
        bodies, _ = kernels(sys.argv[2])
        for sym, body in sorted(bodies.items()):
            text = re.sub(r'\.LBB\d+_', '.LBB_', '\n'.join(body).replace(sym, 'K'))
            print(hashlib.sha1(text.encode()).hexdigest()[:16], len(body), sym)
        return
    bodies, meta = kernels(sys.argv[1])
    for prefix in sys.argv[2:]:
        for sym, body in sorted(bodies.items()):
            if not sym.startswith(prefix):
                continue
            c = {}
            for ins in body:
                k = classify(ins)
                c[k] = c.get(k, 0) + 1
            print(sym)
            print('  static instructions %d: VALU %d (+ v_readlane / v_writelane %d), SALU / SOPP %d, s_waitcnt %d, s_nop %d, scalar loads %d, LDS %d, vector memory %d, other %d' % (
                len(body), c.get('valu', 0), c.get('lane', 0), c.get('salu', 0), c.get('s_waitcnt', 0), c.get('s_nop', 0), c.get('sload', 0), c.get('lds', 0), c.get('vmem', 0), c.get('other', 0)))
            print('  metadata: ' + ', '.join('%s %s' % kv for kv in sorted(meta.get(sym, {}).items())))


if __name__ == '__main__':
    main()
