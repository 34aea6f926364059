#!/usr/bin/env python3
"""Print VGPR / scratch use of every gemv_repacked_kernel<G, T, W, NT, MT, EPI> instantiation (hipcc resource remarks).

The launch heuristic's `rp_fits` table in sglang_awq_amd/csrc/awq_repacked.hip is derived from this output;
run it after touching the kernel.  Exit status 1 if any built instantiation uses scratch.  Also lists the bf16 GEMVs (shared-activation and
straight-line, every (G, T, chunks) of the latter) the bf16 tile kernels by instantiation (dense and AWQ-MoE forms) and the small-group fp16 tile kernels (NJ, GS): the MoE launchers choose their strip widths among the rows without scratch.
"""
import os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "sglang_awq_amd", "csrc", f) for f in ("awq_repacked.hip", "awq_repacked_fused.hip", "awq_repacked_loop.hip", "awq_repacked_sharedx.hip", "awq_repacked_sharedx_wide.hip", "awq_repacked_sharedx_bf16.hip", "awq_repacked_gemv_bf16.hip", "awq_repacked_ext.hip",
                                                                   "awq_repacked_prefill.hip", "awq_repacked_prefill_bf16.hip", "awq_repacked_prefill_sg.hip")]


def main():
    txt = ""
    with tempfile.TemporaryDirectory() as d:
        for src in SRCS:
            cmd = ["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-ffp-contract=on",
                   "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", os.path.join(d, "x.o")]
            txt += subprocess.run(cmd, capture_output=True, text=True, check=True).stderr
    rows = []
    for blk in re.split(r"remark: [^\n]*Function Name: ", txt)[1:]:
        name = blk.split()[0]
        m = re.search(r"gemv_repacked_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb(\d)ELi(\d+)ELi(\d+)E", name)
        if not m:
            continue
        G, T, W, NT, MT, EPI = (int(v) for v in m.groups())
        PRO = 0

        def field(k):
            mm = re.search(k + r": (\d+)", blk)
            return int(mm.group(1)) if mm else -1

        rows.append((PRO, EPI, MT, W, NT, G, T, field("VGPRs"), field(r"ScratchSize \[bytes/lane\]"), field(r"Occupancy \[waves/SIMD\]")))
    rows.sort()
    bad = 0
    for r in rows:
        print("PRO%-2d EPI%d MT%d W%-2d NT%d G%d T%d  vgpr %3d  scratch %4d  occupancy %d" % r)
        bad += r[8] > 0
    print(f"{len(rows)} gemv_repacked_kernel instantiations, {bad} with scratch")
    # the bf16 kernels by instantiation, dense and AWQ-MoE forms (the MoE launchers choose among the strip widths listed here)
    for blk in re.split(r"remark: [^\n]*Function Name: ", txt)[1:]:
        name = blk.split()[0]
        m = re.search(r"gemv_sharedx_bf16_kernelILi(\d+)ELi(\d+)ELb(\d)ELi(\d+)ELb(\d)E", name)
        t = re.search(r"gemm_repacked_pipelined_bf16_kernelILi(\d+)ELb(\d)ELi(\d+)ELb(\d)E", name)
        v = re.search(r"gemv_bf16_kernelILi(\d+)ELi(\d+)ELi(\d+)ELb(\d)E", name)
        g = re.search(r"gemm_repacked_pipelined_sg_kernelILi(\d+)ELi(\d+)E", name)
        if not m and not t and not v and not g:
            continue
        res = tuple(int(re.search(k + r": (\d+)", blk).group(1)) for k in (" VGPRs", r"AGPRs", r"ScratchSize \[bytes/lane\]", r"LDS Size \[bytes/block\]"))
        if g:
            print("tiles_sg NJ%s GS%s  vgpr %3d  agpr %3d  scratch %4d  lds %d" % (g.groups() + res))
        elif v:
            print("gemv_bf16 G%s T%s CHS%s M1_%s  vgpr %3d  agpr %3d  scratch %4d  lds %d" % (v.groups() + res))
        elif m:
            print("sharedx_bf16 G%s MT%s NT%s EPI%s ROWMAP%s  vgpr %3d  agpr %3d  scratch %4d  lds %d" % (m.groups() + res))
        else:
            print("tiles_bf16 NJ%s MOE%s EPI%s SPLIT%s  vgpr %3d  agpr %3d  scratch %4d  lds %d" % (t.groups() + res))
    # every other kernel of these files (gemv_rp2_kernel, gemv_rpx_kernel, the prefill kernels, repack): scratch must be 0 too
    other, other_bad, worst = 0, [], {}
    for blk in re.split(r"remark: [^\n]*Function Name: ", txt)[1:]:
        name = blk.split()[0]
        if "gemv_repacked_kernelI" in name:
            continue
        mm = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", blk)
        vg = re.search(r" VGPRs: (\d+)", blk)
        other += 1
        fam = re.sub(r"I.*", "", name.replace("_ZN3awq", ""))
        worst[fam] = max(worst.get(fam, 0), int(vg.group(1)) if vg else 0)
        if mm and int(mm.group(1)) > 0:
            other_bad.append(name)
    print(f"{other} other kernels, {len(other_bad)} with scratch; max VGPRs per family: " + ", ".join(f"{k} {v}" for k, v in sorted(worst.items())))
    for n in other_bad[:20]:
        print("  scratch:", n)
    return 1 if (bad or other_bad) else 0


if __name__ == "__main__":
    sys.exit(main())
