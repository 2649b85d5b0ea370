#!/usr/bin/env python3
"""Registers / LDS / occupancy of the fused kernels at one line length, from the compiler's own remarks
(-Rpass-analysis=kernel-resource-usage) on a KW_FUSED_ONLY build:  python tools/kernel_resources.py 500"""
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "k-wave-fluid-cuda_amd", "csrc")


def compile_one(args):
    length, src, tmp, extra = args
    cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fvisibility=hidden",
           "-fno-slp-vectorize", f"-DKW_FUSED_ONLY={length}", "-Rpass-analysis=kernel-resource-usage", "-I" + CSRC,
           "-I" + os.path.join(ROOT, "include"), "-I/opt/rocm/include", "-c", src, "-o",
           os.path.join(tmp, os.path.basename(src) + ".o")] + extra
    return subprocess.run(cmd, capture_output=True, text=True).stderr


def main():
    length = int(sys.argv[1]) if len(sys.argv) > 1 else 256
    extra = sys.argv[2:]
    with tempfile.TemporaryDirectory() as tmp, concurrent.futures.ThreadPoolExecutor(8) as pool:
        # the fused pipeline's code objects, and those of the CW propagator and the angular-spectrum projectors (the pair
        # z-pass, the CW projector's y-inverse, the time-domain projector's z-pass, the exact propagator's z-pass k_zfused_second_order and its
        # batched 2-D pass along y k_yfused_second_order, the plane reconstruction's z-pass and
        # the line reconstruction's pass along t are kernels of that pipeline)
        srcs = sorted(glob.glob(os.path.join(CSRC, "kw_fused_*.hip"))) + [os.path.join(CSRC, "kw_cw.hip"),
                                                                          os.path.join(CSRC, "kw_angular.hip"),
                                                                          os.path.join(CSRC, "kw_angular_time.hip"),
                                                                          os.path.join(CSRC, "kw_second_order.hip"),
                                                                          # (the same two passes with dp0/dt)
                                                                          os.path.join(CSRC, "kw_second_order_pair.hip"),
                                                                          # (no kernel of the pipeline: k_line_record<FT>
                                                                          # and k_line_prepare, the same at every length)
                                                                          os.path.join(CSRC, "kw_second_order_line.hip"),
                                                                          # (likewise: k_plane_record<KX>, k_plane_prepare)
                                                                          os.path.join(CSRC, "kw_second_order_plane.hip"),
                                                                          os.path.join(CSRC, "kw_plane_recon.hip"),
                                                                          os.path.join(CSRC, "kw_line_recon.hip")]
        texts = list(pool.map(compile_one, [(length, src, tmp, extra) for src in srcs]))
    pat = re.compile(r"Function Name: (\S+).*?SGPRs: (\d+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?"
                     r"Occupancy \[waves/SIMD\]: (\d+).*?LDS Size \[bytes/block\]: (\d+)", re.S)
    for txt in texts:
        if "error:" in txt:
            print(txt[-3000:])
        for m in pat.finditer(txt):
            dn = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            dn = re.sub(r"\(.*\)$", "", dn.replace("(anonymous namespace)::", "").replace("void ", ""))
            print(f"{dn:52s} sgpr {m.group(2):>3s} vgpr {m.group(3):>4s} agpr {m.group(4):>3s} scratch {m.group(5):>4s} occ {m.group(6)} "
                  f"lds {m.group(7)}")


if __name__ == "__main__":
    main()
