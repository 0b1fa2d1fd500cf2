"""Compare the kernels of two device-only assembly files symbol by symbol.

    hipcc <the Makefile's FLAGS> --cuda-device-only -S csrc/conv_mfma.hip -o a.s    (at each commit)
    python tools/compare_device_asm.py parent.s new.s

A kernel's text is its body (label to end-of-function) plus its .amdhsa_kernel descriptor.  The
function index in local labels (.LBB<i>_<n>, .Lfunc_end<i>) follows the order of emission, which
moves with the order of first use in host code, so it is masked.  Exit status 1 on any difference.
"""
import hashlib
import re
import sys


def kernels(path):
    text = open(path).read()
    names = re.findall(r'^\s*\.amdhsa_kernel\s+(\S+)', text, re.M)
    out = {}
    for n in names:
        body = re.search(r'^%s:.*?^\.Lfunc_end\d+:' % re.escape(n), text, re.M | re.S).group(0)
        desc = re.search(r'^\s*\.amdhsa_kernel\s+%s\n.*?\.end_amdhsa_kernel' % re.escape(n), text,
                         re.M | re.S).group(0)
        body = re.sub(r'\bL?BB\d+_', 'BB_', body)        # labels, and the loop headers in comments
        body = re.sub(r'\.Lfunc_end\d+', '.Lfunc_end', body)
        body = re.sub(r'[ \t]+', ' ', body)              # (comment columns move with a label's width)
        out[n] = (hashlib.sha256((body + desc).encode()).hexdigest()[:16], body.count('\n'))
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    print(f"kernels: {len(a)} / {len(b)}; only in first: {sorted(set(a) - set(b))}; "
          f"only in second: {sorted(set(b) - set(a))}")
    bad += len(set(a) ^ set(b))
    for n in sorted(set(a) & set(b)):
        same = a[n] == b[n]
        bad += not same
        print(f"{'same' if same else 'DIFFERENT'}  {a[n][0]}  {b[n][0]}  {a[n][1]:6d} lines  {n}")
    print(f"{bad} difference(s)")
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
