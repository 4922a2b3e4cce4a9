"""Register / spill / LDS figures of every kernel in libfbr.so (code-object notes).  python tools/kernel_regs.py [family | substring] [lib]
Families: box (csrc/fbr_box.h and the finishing pass it shares), hull (csrc/fbr_hull.h, the frames kernel and the finishing pass it
shares), hullgrad (csrc/fbr_hull_grad.h), mesh (csrc/fbr_mesh.h and the hull
pairs kernel it runs beside), meshgrad (csrc/fbr_mesh_grad.h beside the hull gradient kernel and the mesh pairs kernel), capsule; anything else is matched as a substring."""
import os, re, subprocess, sys, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lib = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "flobaroid_amd", "libfbr.so")
llvm = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
notes = ""
with tempfile.TemporaryDirectory() as td:
    # the fat binaries sit in the .hip_fatbin section of the shared object, one bundle per translation unit
    # (an output file is named so that the library itself is not rewritten in place: its build stamp carries its digest)
    subprocess.check_call([os.path.join(llvm, "llvm-objcopy"), "--dump-section", f".hip_fatbin={td}/fat", lib, f"{td}/lib"])
    with open(f"{td}/fat", "rb") as fh:
        fat = fh.read()
    starts = [m.start() for m in re.finditer(re.escape(MAGIC), fat)]
    for i, a in enumerate(starts):
        with open(f"{td}/fat{i}", "wb") as fh:
            fh.write(fat[a : starts[i + 1] if i + 1 < len(starts) else len(fat)])
        subprocess.check_call([os.path.join(llvm, "clang-offload-bundler"), "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                               f"--input={td}/fat{i}", f"--output={td}/co{i}", "--unbundle"])
        notes += subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", f"{td}/co{i}"], text=True)
pat = re.compile(r"\.agpr_count:\s+(\d+).*?\.group_segment_fixed_size:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.sgpr_count:\s+(\d+).*?\.sgpr_spill_count:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", re.S)
FAMILIES = {"box": ("fbr_box_", "fbr_capsule_finish_kernel"), "hull": ("fbr_hull_", "fbr_box_frames_kernel", "fbr_capsule_finish_kernel"), "hullgrad": ("fbr_hull_grad_kernel",), "mesh": ("fbr_mesh_", "fbr_hull_pairs_kernel"),
            "meshgrad": ("fbr_mesh_grad_", "fbr_hull_grad_kernel", "fbr_mesh_pairs_kernel"), "capsule": ("fbr_capsule_",)}
frag = sys.argv[1] if len(sys.argv) > 1 else ""
frags = FAMILIES.get(frag, (frag,))
for m in pat.finditer(notes):
    agpr, lds, name, priv, sgpr, sspill, vgpr, vspill = m.groups()
    try:
        name = subprocess.check_output(["c++filt", name], text=True).strip()
    except Exception:
        pass
    if any(f in name for f in frags):
        print(f"vgpr={vgpr:>3} agpr={agpr:>3} vspill={vspill:>3} sgpr={sgpr:>3} sspill={sspill:>3} scratch={priv:>5} lds={lds:>6}  {name[:110]}")
