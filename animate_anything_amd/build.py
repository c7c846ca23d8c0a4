"""Build libaa_mi355.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
import os
import subprocess

PKG = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(PKG)
CSRC = os.path.join(PKG, "csrc")
LIB = os.path.join(PKG, "libaa_mi355.so")


def _deps():
    deps = [os.path.join(ROOT, "include", "aa_mi355.h")]
    for d, _, fs in os.walk(CSRC):
        deps += [os.path.join(d, f) for f in fs if f.endswith((".h", ".hip"))]
    return deps


def source_id():
    """sha256[:16] over the library's sources (csrc/**, include/aa_mi355.h, in path order): names WHAT was built, wherever and whenever it is
    rebuilt - bench.py quotes a committed PMC record only for the sources it was measured on."""
    import hashlib
    h = hashlib.sha256()
    for d in sorted(_deps()):
        h.update(os.path.relpath(d, ROOT).encode())
        h.update(open(d, "rb").read())
    return h.hexdigest()[:16]


PROBE_LIB = os.path.join(PKG, "libaa_mi355_probe.so")
TU_GROUPS = 8             # aa_api_impl.h: tile-table entry i is compiled in unit i % TU_GROUPS


def build(force=False, verbose=False, probe=False, ablate=0, variant=None):
    """Compile csrc/aa_api.hip + 8 x csrc/aa_tiles.hip -> libaa_mi355.so (skipped when up to date). Returns the path.
    probe=True builds the -DAA_PHASE_PROBE profiling variant (scripts/phase_probe.py) next to it;
    ablate=bits a timing-only -DAA_X_ABLATE variant of the hand-scheduled kernels (scripts/x_ablate.py)."""
    LIB = PROBE_LIB if probe else globals()["LIB"]
    if ablate:
        LIB = os.path.join(PKG, f"libaa_mi355_abl{ablate}.so")
    if variant:                                             # (name, [-D...]): an A/B build next to the library, loaded through AA_LIBRARY
        LIB = os.path.join(PKG, f"libaa_mi355_{variant[0]}.so")
    if not force and os.path.exists(LIB) and all(os.path.getmtime(LIB) >= os.path.getmtime(d) for d in _deps()):
        return LIB
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffast-math", f"-DAA_TU_GROUPS={TU_GROUPS}",
             "-I", os.path.join(CSRC, "kernels", "device"), "-I", os.path.join(CSRC, "kernels"), "-I", CSRC,
             "-I", os.path.join(ROOT, "include")]
    if probe:
        flags.insert(0, "-DAA_PHASE_PROBE")
    if ablate:
        flags.insert(0, f"-DAA_X_ABLATE={int(ablate)}")
    if variant:
        flags = list(variant[1]) + flags
    if verbose:
        flags.insert(0, "-Rpass-analysis=kernel-resource-usage")
    # one translation unit for the C ABI + TU_GROUPS units with a slice of the contraction tile table each, compiled in parallel
    # (a single unit took more than five minutes), linked into one shared object
    obj_dir = os.path.join(PKG, "build", os.path.basename(LIB)[:-3])
    os.makedirs(obj_dir, exist_ok=True)
    jobs = [([os.path.join(CSRC, "aa_api.hip")], os.path.join(obj_dir, "aa_api.o"))]
    jobs += [([f"-DAA_TU_GROUP={g}", os.path.join(CSRC, "aa_tiles.hip")], os.path.join(obj_dir, f"aa_tiles_{g}.o")) for g in range(TU_GROUPS)]

    # Incremental: an object is recompiled only when the sources it can see changed.  The tile units (aa_tiles.hip) include the
    # attention / norm / glue kernels' headers through aa_api_impl.h but instantiate nothing of them (AA_TU_TILES_ONLY), so edits
    # there rebuild the C-ABI unit alone (~1.5 of the ~4 minutes).  Key = sha256 of (flags, the unit's sources).
    import hashlib
    api_only = {"attention.h", "seq_attention.h", "norm.h", "glue.h", "freeu.h", "cfg_rescale.h", "apg.h", "window.h", "freeinit.h", "keep.h", "ff_fused.h", "linear_rows.h", "linear_fp8.h"}

    def dep_hash(job):
        src, _ = job
        h = hashlib.sha256(repr((flags, [x for x in src if x.startswith("-D")])).encode())
        tiles = any("aa_tiles.hip" in x for x in src)
        for d in sorted(_deps()):
            if tiles and (os.path.basename(d) in api_only or d.endswith("aa_api.hip")):
                continue
            if not tiles and d.endswith("aa_tiles.hip"):
                continue
            h.update(d.encode())
            h.update(open(d, "rb").read())
        return h.hexdigest()

    def compile_one(job):
        src, obj = job
        key, stamp = dep_hash(job), obj + ".dephash"
        if not force and os.path.exists(obj) and os.path.exists(stamp) and open(stamp).read() == key:
            return obj
        subprocess.check_call([hipcc] + flags + ["-c"] + src + ["-o", obj])
        with open(stamp, "w") as f:
            f.write(key)
        return obj

    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=max(1, min(len(jobs), os.cpu_count() or 1))) as pool:
        objs = list(pool.map(compile_one, jobs))
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs + ["-o", LIB])
    # The hand-scheduled kernels keep their accumulators under literal register names hipcc does not manage: whether a build is sound
    # depends on what THIS compiler did around them, so the code-object audit is part of the build, and the compiler that
    # produced the library is recorded next to it.
    import shutil
    have_tools = shutil.which(os.path.join(LLVM_TOOLS, "llvm-objdump")) and shutil.which(os.path.join(LLVM_TOOLS, "llvm-readelf"))
    if not ablate and os.environ.get("AA_BUILD_AUDIT", "1") != "0" and not have_tools:
        import json
        with open(LIB[:-3] + ".buildinfo.json", "w") as f:       # (a toolchain without the LLVM binutils: built, NOT audited - say so)
            json.dump({"flags": flags, "audit": "skipped: llvm-objdump / llvm-readelf not found under " + LLVM_TOOLS}, f, indent=1)
    elif not ablate and os.environ.get("AA_BUILD_AUDIT", "1") != "0":
        problems = audit_x_kernels(LIB)
        info = {"hipcc": subprocess.run([hipcc, "--version"], capture_output=True, text=True).stdout.strip().split("\n"),
                "flags": flags, "audit": "ok" if not problems else problems}
        import json
        with open(LIB[:-3] + ".buildinfo.json", "w") as f:
            json.dump(info, f, indent=1)
        if problems:
            os.replace(LIB, LIB + ".rejected")
            raise RuntimeError("libaa_mi355.so: the code-object audit of the hand-scheduled kernels failed (library moved to "
                               + LIB + ".rejected):\n  " + "\n  ".join(str(p_) for p_ in problems[:8]))
    return LIB


LLVM_TOOLS = "/opt/rocm/lib/llvm/bin"


def device_code_objects(lib_path, out_dir):
    """The gfx950 code objects inside the library: one clang offload bundle per translation unit (csrc/aa_api.hip and the groups of
    csrc/aa_tiles.hip), written to `out_dir`; returns their paths."""
    import struct
    data = open(lib_path, "rb").read()
    out, start = [], 0
    while True:
        i = data.find(b"__CLANG_OFFLOAD_BUNDLE__", start)
        if i < 0:
            break
        start = i + 24
        n = struct.unpack_from("<Q", data, i + 24)[0]
        if not 0 < n < 16:
            continue
        off = i + 32
        for _ in range(n):
            o, s_, ln = struct.unpack_from("<QQQ", data, off)
            off += 24
            name = data[off:off + ln].decode(errors="replace")
            off += ln
            if "gfx950" in name and s_ > 0:
                p = os.path.join(out_dir, f"dev{len(out)}.co")
                with open(p, "wb") as f:
                    f.write(data[i + o:i + o + s_])
                out.append(p)
    return out


def audit_x_kernels(lib_path):
    """Audit of the hand-scheduled contraction kernels (csrc/kernels/conv_gemm_x.h) in a built library; returns a list of problems
    (empty = sound).  Those kernels name their accumulators a[0:255] literally; hipcc does not know the registers are live, so it must
    neither spill (scratch) nor touch accumulation registers itself (cdna guide 5.7 item 4).  Per kernel: no private segment, no
    VGPR spills, a register count that fits its waves per SIMD, exactly the v_accvgpr traffic the source writes (16 initialising
    writes per literal block and site, whole-block reads per read-out site), every MFMA with an a[...] destination one of the source's
    literal statements (destination = third source, aligned to a block, inside the literal range - round 4 had the MFMA builtin of
    the row-statistics epilogue reuse literal blocks), and no other instruction naming an accumulation register."""
    import re
    import shutil
    import tempfile
    if not shutil.which(os.path.join(LLVM_TOOLS, "llvm-objdump")):
        return ["llvm-objdump / llvm-readelf not found under " + LLVM_TOOLS + ": the library cannot be audited"]
    problems = []
    with tempfile.TemporaryDirectory() as tmp:
        cos = device_code_objects(lib_path, tmp)
        if not cos:
            return ["no gfx950 code object in " + lib_path]
        run = lambda *a: subprocess.run(list(a), capture_output=True, text=True, check=True).stdout
        notes = "".join(run(os.path.join(LLVM_TOOLS, "llvm-readelf"), "--notes", co) for co in cos)
        dis = "".join(run(os.path.join(LLVM_TOOLS, "llvm-objdump"), "-d", "--no-show-raw-insn", co) for co in cos)
    meta = {}
    for m in re.finditer(r"\.agpr_count:\s+(\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size:\s+(\d+).*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count:\s+(\d+)", notes, re.S):
        meta[m.group(2)] = tuple(int(m.group(k)) for k in (1, 3, 4, 5))
    # the attention / GroupNorm kernels must not spill either (some wide compiled contraction tiles do - the autotuner never picks them): round 5 first kept the attention scores alive across a test and hipcc spilled 18
    # registers into the key loop at the kernel's 168-register cap - the 4096-key kernel ran 55 % slower and nothing said so
    for k, (_agpr, scratch, _vgpr, spills) in sorted(meta.items()):
        # (the one-wave-per-SIMD instances of seq_self_attention_kernel hold x in the upper half of the 512-register file: hipcc reports the
        #  copies into accumulation registers as VGPR spills - scratch is what must not appear there)
        upper_half_ok = "seq_self_attention_kernel" in k and _agpr > 0
        if any(t in k for t in ("attention_kernel", "attention_shortkv_kernel", "groupnorm_")) and (scratch or (spills and not upper_half_ok)):
            problems.append(f"{k}: scratch {scratch} bytes, {spills} VGPR spills in a hot kernel")
    # the one-wave-per-SIMD FeedForward kernel lives at the edge of the register file too: no scratch, no spills (its ablation instantiations
    # are profiling code and exempt)
    for k, (_agpr, scratch, _vgpr, spills) in sorted(meta.items()):
        if ("ff_fused_kernel" in k and "ELi0EEE" in k or "linear_rows_kernel" in k or "linear_fp8_kernel" in k or "quant_rows_fp8_kernel" in k) and (scratch or spills):
            problems.append(f"{k}: scratch {scratch} bytes, {spills} VGPR spills in a hot kernel")
    xk = {k: v for k, v in meta.items() if "conv_gemm_x_kernel" in k or "conv_gemm_x_group_kernel" in k}      # (the grouped launch runs the same body)
    if len(xk) < 16:                                        # 8 tiles x {fp16, bf16} at the very least
        problems.append(f"only {len(xk)} hand-scheduled kernels found")
    bodies, cur = {}, None
    for line in dis.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            cur = m.group(1)
            bodies[cur] = []
        elif cur is not None:
            bodies[cur].append(line)
    # Hand-issued LDS reads (dev.h lds_read16_async*, lds_read_tr16_b64_async: `asm volatile` with an "=v" output): hipcc believes the
    # destination is valid right behind the statement, the data arrives at the matching counted s_waitcnt.  Nothing may name such a register
    # in between (a live-range split or a v_mov there would copy stale data - ADVICE r05).  Linear walk per kernel: LDS operations retire in
    # order, `s_waitcnt lgkmcnt(N)` leaves at most N of them pending (scalar loads also count in the hardware counter: ignoring them is the
    # conservative reading).
    for name in sorted(bodies):
        if not any(t in name for t in ("attention_kernel", "attention_shortkv_kernel", "ff_fused_kernel", "linear_rows_kernel", "linear_fp8_kernel")):
            continue
        hit = pending_lds_read_violation(bodies[name])
        if hit:
            problems.append(f"{name}: {hit}")
    for name, (agpr, scratch, vgpr, spills) in sorted(xk.items()):
        bad = lambda what: problems.append(f"{name}: {what}")
        if scratch or spills:
            bad(f"scratch {scratch} bytes, {spills} VGPR spills")
        m = re.search(r"x_(?:group_)?kernelI\w+?Li(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", name)
        if m is None or name not in bodies:                  # another mangling / template parameter list, or no disassembly: not auditable
            bad("cannot parse the kernel name" if m is None else "no disassembly found")
            continue
        wm, wn, per_cu = int(m.group(3)), int(m.group(4)), int(m.group(10))
        waves_per_simd = wm * wn * per_cu // 4             # 1: the whole 512-register file per lane; 2: half of it
        if vgpr > 512 // waves_per_simd:
            bad(f"{vgpr} registers per lane at {waves_per_simd} waves per SIMD")
        body = "\n".join(bodies.get(name, []))
        literal_blocks = agpr // 16
        if literal_blocks not in (4, 8, 12, 15, 16):
            bad(f"{agpr} accumulation registers")
            continue
        # written by the source only: started from the bias (or a folded LayerNorm's terms) at the K loop prologue / empty K range
        # (the BK = 64 prologue has two sites, tiles that can start from a folded LayerNorm two forms per site)
        writes = len(re.findall(r"v_accvgpr_write", body))
        if writes % (16 * literal_blocks) or not 2 <= writes // (16 * literal_blocks) <= 8:
            bad(f"{writes} v_accvgpr_write for {literal_blocks} literal blocks (hipcc parked values in accumulation registers)")
        # read-out sites (split-K partials, the general epilogue, its branch-free forms, the in-kernel K-split finish) read whole blocks
        reads = len(re.findall(r"v_accvgpr_read", body))
        if not 2 * 16 * literal_blocks <= reads <= 32 * 16 * literal_blocks:
            bad(f"{reads} v_accvgpr_read for {literal_blocks} literal blocks")
        if "scratch_" in body:
            bad("scratch access")
        for d, c in re.findall(r"v_mfma_f32_32x32x16_\w+\s+([av]\[\d+:\d+\]),\s*\S+,\s*\S+,\s*([av]\[\d+:\d+\]|\S+)", body):
            if d.startswith("a"):
                lo = int(re.match(r"a\[(\d+):", d).group(1))
                if d != c or lo % 16 or lo >= 16 * literal_blocks:
                    bad(f"MFMA with accumulation-register destination {d} (third source {c}) is not one of the source's statements")
        for line in bodies.get(name, []):
            if re.search(r"[\s,]a(\[\d+:\d+\]|\d+)\b", line) and not re.search(r"^\s*(v_mfma_|v_accvgpr_)", line.strip()):
                bad("accumulation register outside the source's statements: " + line.strip())
                break
    return problems


def _vregs(tok):
    """'v[4:7]' -> {4,5,6,7}; 'v12' -> {12}; anything else -> empty."""
    import re
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r"v(\d+)", tok)
    return {int(m.group(1))} if m else set()


def pending_lds_read_violation(lines):
    """First instruction of a disassembled kernel body that names the destination of an LDS read which no s_waitcnt has retired yet
    (None if there is none).  See audit_x_kernels."""
    import re
    pending = []                                            # destination register sets of LDS operations in issue order (empty set: a store)
    for raw in lines:
        line = raw.strip()
        if not line or line.startswith(("//", ";")):
            continue
        ins = line.split("//")[0].strip()
        op = ins.split()[0] if ins.split() else ""
        toks = [t.strip() for t in re.split(r"[\s,]+", ins)[1:] if t.strip()]
        if op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", ins)
            if m:
                keep = int(m.group(1))
                pending = pending[len(pending) - keep:] if keep else []
            continue
        named = set()
        for t in toks:
            named |= _vregs(t)
        busy = set().union(*pending) if pending else set()
        if op.startswith("ds_"):
            dst = _vregs(toks[0]) if toks and op.startswith(("ds_read", "ds_load", "ds_bpermute", "ds_permute", "ds_swizzle")) else set()
            # (its own destination may be one that is still pending: LDS returns in order, the later write wins; its ADDRESS must not be pending)
            if (named - dst) & busy:
                return "LDS access uses a register whose LDS read has not been waited for: " + ins
            pending.append(dst)
            continue
        if named & busy:
            return "register of an LDS read that has not been waited for is used: " + ins
    return None


if __name__ == "__main__":
    import sys
    print(build(force=True, verbose="-v" in sys.argv, probe="--probe" in sys.argv))
