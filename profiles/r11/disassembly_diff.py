"""Per-kernel comparison of two trees' device assembly (`hipcc <the Makefile rule's flags> -S --cuda-device-only -c X.hip -o DIR/X.s`):
    python disassembly_diff.py PARENT_DIR CANDIDATE_DIR m2s_fused3 m2s_fused2 ...
Instruction lines only (comments, directives and metadata dropped); the kernel's own name and the per-function label numbers are normalised."""
import re, sys, collections
def funcs(path):
    out = collections.OrderedDict()
    cur = None
    for line in open(path):
        m = re.match(r'^(_Z\w+|\w+):\s*(;.*)?$', line)
        if m and not line.startswith('.L'):
            cur = m.group(1); out[cur] = []; continue
        if cur is None: continue
        s = line.strip()
        if s.startswith('.Lfunc_end'):
            cur = None; continue
        if not s or s.startswith(';') or s.startswith('.') and not s.startswith('.LBB'): continue
        s = re.sub(r'\s*;.*$', '', s)
        out[cur].append(s)
    return out
def norm(name):   # the second template argument of k_fused3 and its last parameter are new: <x, false> is the parent's <x>
    m = re.match(r'_ZN3m2s8k_fused3I(Lb[01]E)(Lb0E)?EEvNS_8SceneDev', name)
    return 'k_fused3<%s>' % m.group(1) if m else name
PARENT, CAND = sys.argv[1:3]
for f in sys.argv[3:]:
    a = funcs('%s/%s.s' % (PARENT, f)); b = funcs('%s/%s.s' % (CAND, f))
    bn = {norm(k): (k, v) for k, v in b.items()}; a = collections.OrderedDict((norm(k), (k, v)) for k, v in a.items())
    print('== %s.hip' % f)
    for k, (pk, v) in a.items():
        if k.startswith('__hip_cuid'): continue
        if k not in bn: print('  %-60s parent only' % k[:60]); continue
        ck, cv = bn[k]
        def body(name, lines): return [re.sub(r'\.LBB\d+_', '.LBB_', l.replace(name, 'K')) for l in lines]   # (labels carry the function's index in its file)
        same = body(pk, v) == body(ck, cv)
        valu = sum(1 for l in v if l.startswith('v_'))
        print('  %-60s %6d lines %6d v_*  %s' % (k[:60], len(v), valu, 'IDENTICAL' if same else 'DIFFERS (%d lines in candidate)' % len(cv)))
    for k, (ck, cv) in bn.items():
        if k not in a and not k.startswith('__hip_cuid'): print('  %-60s candidate only: %d lines, %d v_*' % (ck[:60], len(cv), sum(1 for l in cv if l.startswith('v_'))))
