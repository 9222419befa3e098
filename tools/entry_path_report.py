#!/usr/bin/env python3
"""Entry path of the decode step's kernels, read from their gfx950 assembly (CPU only: needs hipcc, no GPU).

The entry contract: the values a kernel's first vector loads are built from lead its parameter list and
are preloaded into SGPRs at wave launch, so those loads are issued without a scalar round trip to the kernarg segment or to a
device word.  For each kernel instance of a generation step (bench.py step_launches names them) this prints

    preload   .amdhsa_user_sgpr_kernarg_preload_length: dwords of leading parameters the hardware puts into SGPRs
    waits     s_waitcnt instructions that name lgkmcnt between the preloaded entry and the reference load - each one is a
              scalar (or LDS) round trip in front of the stream
    pos       the reference load's position, in instructions from the preloaded entry
    first     position of the first vector load of any kind (x, gamma, logits)

The reference load is the first non-temporal 16-byte load (the weight stream: dev::ld_nt16) or, for the kernels without a weight
stream (the sampler), the first vector load: its logits.  The "preloaded entry" is what a wave runs when the firmware preloads:
the compatibility prologue in front of it (s_load of the same dwords, s_waitcnt, s_branch, padded to 256 bytes) is skipped.

    python tools/entry_path_report.py            # the SmoothQuant step
    python tools/entry_path_report.py --json
"""
import argparse
import json
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'trtllm-llama_amd', 'csrc')

# (key, translation unit, kernel as rocprofv3 / bench.py print it)
SQ_STEP = [
    ('front', 'kernels/qkv_attn_fused.hip', 'qkv_attn_fused_kernel<3, true, 0>'),
    ('gate_up', 'kernels/gemv_sq.hip', 'gemv_kernel<3, 1, 1, 1, 2, 4>'),
    ('down', 'kernels/gemv_ksplit.hip', 'gemv_ksplit_kernel<3, 3>'),
    ('head', 'kernels/gemv_fp16.hip', 'gemv_kernel<0, 1, 0, 1, 2, 4>'),
    ('sampler', 'kernels/decode_step.hip', 'greedy_step_kernel'),
]


def hipcc():
    return os.environ.get('HIPCC') or shutil.which('hipcc') or ('/opt/rocm/bin/hipcc' if os.path.exists('/opt/rocm/bin/hipcc') else None)


def unit_flags(unit):
    """The flags csrc/Makefile gives this translation unit, read from its text: CXXFLAGS, the architecture and - for the units it
    lists in PRELOAD_UNITS - the per-unit options of the rule that names that list."""
    mk = open(os.path.join(CSRC, 'Makefile')).read()
    var = lambda name: re.search(r'^%s\s*[:?]?=\s*(.*)$' % name, mk, re.M).group(1).split()
    flags = ['--offload-arch=' + var('ARCH')[0]] + [f for f in var('CXXFLAGS') if f != '-fPIC']
    if os.path.basename(unit)[:-4] in var('PRELOAD_UNITS'):
        flags += re.search(r'\$\(PRELOAD_UNITS\).*HIPFLAGS \+= ([^)]*)\)\)', mk).group(1).split()
    return flags + ['-x', 'hip']


def assemble(unit, outdir, flags=None):
    dst = os.path.join(outdir, os.path.basename(unit)[:-4] + '.s')
    cmd = [hipcc()] + (unit_flags(unit) if flags is None else flags) + ['-S', '--cuda-device-only', unit, '-o', dst]
    subprocess.run(cmd, check=True, cwd=CSRC, capture_output=True, text=True)
    return dst


def mangled_pattern(kernel):
    """'gemv_kernel<3, 1, 1, 1, 2, 4>' -> regex on the Itanium name (integers as Li<n>E, bools as Lb<0|1>E)."""
    m = re.match(r'(\w+)(?:<(.*)>)?$', kernel)
    name, targs = m.group(1), m.group(2)
    pat = r'%d%s' % (len(name), name)
    if targs:
        pat += 'I'
        for a in [t.strip() for t in targs.split(',')]:
            pat += {'true': 'Lb1E', 'false': 'Lb0E'}.get(a, 'Li%sE' % a)
        pat += 'E'
    return re.compile(pat if targs else pat + '(?!I)')


def kernel_text(asm, kernel):
    """(instructions of the kernel as a list, its .amdhsa_kernel descriptor text)"""
    pat = mangled_pattern(kernel)
    sym = None
    for m in re.finditer(r'^\s*\.amdhsa_kernel (\S+)$', asm, re.M):
        if pat.search(m.group(1)):
            sym = m.group(1)
            break
    if sym is None:
        raise KeyError('no kernel %r in the assembly' % kernel)
    start = asm.index('\n' + sym + ':')
    end = asm.index('.Lfunc_end', start)
    desc_at = asm.index('.amdhsa_kernel ' + sym)
    desc = asm[desc_at:asm.index('.end_amdhsa_kernel', desc_at)]
    ins = []
    for line in asm[start:end].splitlines()[2:]:
        line = line.split(';')[0].strip()
        if not line or line.endswith(':'):
            continue
        if line.startswith('.'):
            if line.startswith('.p2align') and ins:
                ins.append(line)  # the end of the compatibility prologue
            continue
        ins.append(line)
    return ins, desc


def entry_path(ins, desc):
    preload = int(re.search(r'\.amdhsa_user_sgpr_kernarg_preload_length (\d+)', desc).group(1))
    body = ins
    if preload:
        # s_load ... ; s_waitcnt lgkmcnt(0) ; s_branch ; .p2align 8 ; <preloaded entry>
        cut = [i for i, l in enumerate(ins[:16]) if l.startswith('.p2align')]
        assert cut and any(l.startswith('s_branch') for l in ins[:cut[0]]), 'preload without the compatibility prologue'
        body = ins[cut[0] + 1:]
    body = [l for l in body if not l.startswith('.')]
    vec = [i for i, l in enumerate(body) if re.match(r'(global|flat|buffer)_load', l)]
    nt = [i for i in vec if re.search(r'\bnt\b', body[i])]
    first = vec[0]
    ref = nt[0] if nt else first
    waits = [i for i, l in enumerate(body[:ref]) if l.startswith('s_waitcnt') and 'lgkmcnt' in l]
    waits_first = [i for i in waits if i < first]
    return dict(preload=preload, waits=len(waits), pos=ref, first=first, waits_first=len(waits_first), kind='weight' if nt else 'first')


def report(step=SQ_STEP, flags=None):
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        cache = {}
        for key, unit, kernel in step:
            if unit not in cache:
                cache[unit] = open(assemble(unit, tmp, flags)).read()
            ins, desc = kernel_text(cache[unit], kernel)
            rows.append(dict(key=key, unit=unit, kernel=kernel, **entry_path(ins, desc)))
    return rows


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--json', action='store_true')
    ap.add_argument('--plain-flags', action='store_true', help='compile without the per-unit options of csrc/Makefile (no preload)')
    args = ap.parse_args()
    if not hipcc():
        sys.exit('hipcc not found')
    flags = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-I/opt/rocm/include', '-x', 'hip'] if args.plain_flags else None
    rows = report(flags=flags)
    if args.json:
        print(json.dumps(rows))
        return
    print('%-8s %-36s %8s %6s %6s %6s  %s' % ('launch', 'kernel', 'preload', 'waits', 'pos', 'first', 'reference load'))
    for r in rows:
        print('%-8s %-36s %8d %6d %6d %6d  %s' % (r['key'], r['kernel'], r['preload'], r['waits'], r['pos'], r['first'], r['kind']))


if __name__ == '__main__':
    main()
