"""launch_igemm's routing decision on the CPU: csrc/igemm_plan.h (igemm_plan: validation, kernel family and instantiation, launch geometry) driven through the
stand-alone program tests/sanitize/igemm_plan_harness.cpp, compiled host-only with -fsanitize=address,undefined (hipcc --cuda-host-only; nothing is preloaded).
Every non-null pointer the harness passes points into poisoned memory, so a plan that dereferenced one (it may only test them for null) is a sanitizer error.

Three groups of cases, each compared with the route it already carries:
  1. every case of tests/igemm_ref.py (ALL_CONV_CASES, SUB_CASES, LINEAR_ROUTES x LINEAR_M x LINEAR_K, GEGLU_ROUTES): the routes tests/test_igemm_forms_gpu.py asserts
     on the GPU after the launch are asserted here before any launch;
  2. the refusals of test_refusals_leave_the_output_untouched that the launcher makes (the others are the C entry points'), by their error codes;
  3. SD15_ROUTES: every distinct launch_igemm call of the SD1.5 UNet at batch 2 and batch 32 and of the VAE decoder at 64 x 64 latents under the default knobs, with
     the route the launcher took for it BEFORE the routing became a pure function (recorded from that version of launch_igemm compiled host-only).
For every case the invariants a launch relies on: dynamic LDS within the 160 KiB of a CU, a non-empty grid, the variant inside its table, tile columns that divide N
(GEGLU: half a tile divides the N / 2 output columns), gridDim.y = splits, and split-K partial sums that fit the scratch the caller gave.

The numbering of the variants: the enums and index functions of csrc/igemm_plan.h (IgemmKernelForm / IK_VARIANT, ConvLwVariant, SubVariant, W8Variant, GemmLwVariant,
AsVariant).
"""
import os
import shutil
import subprocess

import pytest

from tests import igemm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CS_OK, CS_E_ARG, CS_E_SHAPE = 0, -1, -2
FAMILIES = ("none", "generic", "halo", "conv3_lw", "sub_pixel", "gemm_big", "gemm_w8", "gemm_lw", "gemm_as")      # consolver_amd.ops.IGEMM_FAMILIES
# pointer_mask bits, in the order of the harness's PTR enum
PTRS = ("a0", "w", "out", "a1", "bias", "temb", "res", "res_lo", "out_lo", "a0_lo", "a1_lo", "row_stats", "row_stats_groups", "gn_stats", "ln_stats", "ln_s", "ln_b", "w_up_sub",
        "splitk_ws")
SPLITK_WS_BYTES = 64 << 20           # consolver_amd.ops: the scratch conv2d passes for 3x3 convs
# family -> (variants the record may hold, entries of the family's kernel table)
TABLES = {1: ({0, 1, 2, 4, 6, 16, 17, 32}, 14), 2: ({0, 1}, 8), 3: (set(range(11)), 11), 4: (set(range(3)), 3), 5: ({0, 1}, 3), 6: (set(range(8)), 8), 7: (set(range(6)), 6),
          8: (set(range(4)), 4)}


def mask(*names):
    return sum(1 << PTRS.index(n) for n in ("a0", "w", "out") + names)


def line(B, Hi, Wi, Ho, Wo, c0, c1, taps, stride, up, pad_after_only, N, ptrs, geglu=0, lo8=0, ln_groups=0, ws_bytes=0, knobs=()):
    v = [B, Hi, Wi, Ho, Wo, c0, c1, taps, stride, int(up), int(pad_after_only), N, geglu, lo8, ln_groups, ptrs, ws_bytes]
    return " ".join(str(x) for x in v) + "".join(f" {k} {x}" for k, x in knobs)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    hipcc = next((c for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")) if c and os.path.exists(c)), None)
    if hipcc is None:
        pytest.skip("hipcc not found")
    exe = str(tmp_path_factory.mktemp("igemm_plan") / "igemm_plan_harness")
    cmd = [hipcc, "-x", "hip", "--cuda-host-only", "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-gpu-sanitize",
           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-w", "-I" + os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "sanitize", "igemm_plan_harness.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr

    def run(lines):
        """-> one dict per line: rc, the route fields, slot, grid_x, grid_y, block, lds, splitk_bytes, error"""
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
        p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env=env, timeout=120)
        text = p.stdout + p.stderr
        assert p.returncode == 0 and "AddressSanitizer" not in text and "runtime error" not in text, text[-4000:]
        rows = p.stdout.splitlines()
        assert len(rows) == len(lines)
        keys = ("rc", "family", "tile_cols", "variant", "splits", "gn_done", "row_groups", "slot", "grid_x", "grid_y", "block", "lds", "splitk_bytes")
        out = []
        for row in rows:
            nums, _, err = row.partition(" | ")
            out.append(dict(zip(keys, (int(x) for x in nums.split())), error=err))
        return out
    return run


def check_invariants(ln, got):
    """what a launch of the plan relies on; ln: the case's input line"""
    v = ln.split()
    N, geglu, ptrs, ws_bytes = int(v[11]), int(v[12]), int(v[15]), int(v[16])
    if got["rc"] != CS_OK or got["family"] == 0:
        assert got["family"] == 0 and got["splitk_bytes"] == 0, (ln, got)
        assert got["rc"] == CS_OK or got["error"] or int(v[0]) < 0, (ln, got)          # a refusal says why (B < 0 alone is a bare CS_E_SHAPE)
        return
    variants, entries = TABLES[got["family"]]
    assert got["variant"] in variants and 0 <= got["slot"] < entries, (ln, got)
    assert 0 < got["lds"] <= 160 * 1024, (ln, got)
    assert got["grid_x"] > 0 and got["grid_y"] > 0 and got["block"] in (256, 512) and got["grid_y"] == got["splits"], (ln, got)
    cols = got["tile_cols"]
    assert cols > 0 and N % cols == 0, (ln, got)
    if geglu:
        assert cols % 2 == 0 and (N // 2) % (cols // 2) == 0, (ln, got)
    if got["splits"] > 1:
        assert ptrs >> PTRS.index("splitk_ws") & 1 and 0 < got["splitk_bytes"] <= ws_bytes, (ln, got)
    else:
        assert got["splitk_bytes"] == 0, (ln, got)


def expect_route(ln, got, family, cols=None, variant=None, splits=None, gn_done=None, row_groups=None):
    assert got["rc"] == CS_OK, (ln, got)
    want = dict(family=family, tile_cols=cols, variant=variant, splits=splits, gn_done=gn_done, row_groups=row_groups)
    bad = {k: (got[k], w) for k, w in want.items() if w is not None and got[k] != w}
    assert not bad, f"{ln}: (got, want) {bad}"


def conv_line(c):
    """a tests/igemm_ref.py ConvCase as consolver_amd.ops.conv2d / conv_down hands it to the library"""
    Ho, Wo = c.out_hw
    down = c.api == "conv_down"
    names = (("a1",) if c.c1 else ()) + (("bias",) if c.bias else ()) + (("temb",) if c.temb else ()) + (("res",) if c.res else ()) + (("gn_stats",) if c.gn else ())
    ws = c.splitk and c.taps == 9 and not down
    return line(c.B, c.H, c.W, Ho, Wo, c.c0, c.c1, c.taps, c.stride, c.up, down, c.N, mask(*names, *(("splitk_ws",) if ws else ())), ws_bytes=SPLITK_WS_BYTES if ws else 0,
                knobs=c.knobs)


def test_conv_cases_of_igemm_ref(harness):
    lines = [conv_line(c) for c in R.ALL_CONV_CASES]
    for c, ln, got in zip(R.ALL_CONV_CASES, lines, harness(lines)):
        expect_route(ln, got, FAMILIES.index(c.family), c.cols, c.variant, c.splits, c.gn_done)
        check_invariants(ln, got)


def test_sub_pixel_cases_of_igemm_ref(harness):
    lines = [line(B, Hi, Wi, 2 * Hi, 2 * Wi, cin, 0, 9, 1, 1, 0, N, mask("bias", "gn_stats", "w_up_sub")) for B, Hi, Wi, cin, N, _ in R.SUB_CASES]
    for (_, _, _, _, _, idx), ln, got in zip(R.SUB_CASES, lines, harness(lines)):
        expect_route(ln, got, FAMILIES.index("sub_pixel"), 128 if idx == 2 else 160, idx, 1, 1, 0)
        check_invariants(ln, got)


def test_linear_and_geglu_routes_of_igemm_ref(harness):
    lines, want = [], []
    for kn, N, fam, cols, variant in R.LINEAR_ROUTES.values():
        i = 0
        for K in R.LINEAR_K:
            for M in R.LINEAR_M:                                      # bias / residual / nothing rotating, as test_linear_routes_at_every_row_edge
                names = (("bias",) if i % 3 != 2 else ()) + (("res",) if i % 3 == 1 else ())
                lines.append(line(1, M, 1, M, 1, K, 0, 1, 1, 0, 0, N, mask(*names), knobs=kn))
                want.append((fam, cols, variant))
                i += 1
    for kn, N, fam, cols, variant in R.GEGLU_ROUTES:
        for M in (1, 65, 257, 321):
            for K in (64, 320):
                lines.append(line(1, M, 1, M, 1, K, 0, 1, 1, 0, 0, N, mask("bias"), geglu=1, knobs=kn))
                want.append((fam, cols, variant))
    for (fam, cols, variant), ln, got in zip(want, lines, harness(lines)):
        expect_route(ln, got, FAMILIES.index(fam), cols, variant, 1)
        check_invariants(ln, got)


def test_refusals_by_error_code(harness):
    """the launcher's refusals of test_refusals_leave_the_output_untouched (tests/test_igemm_forms_gpu.py): the record stays at family 0"""
    cases = [("N = 192", line(1, 8, 8, 8, 8, 64, 0, 9, 1, 0, 0, 192, mask()), CS_E_SHAPE),
             ("c0 = 32", line(1, 8, 8, 8, 8, 32, 0, 9, 1, 0, 0, 128, mask()), CS_E_SHAPE),
             ("taps 1 with stride 2", line(1, 8, 8, 4, 4, 64, 0, 1, 2, 0, 0, 128, mask()), CS_E_ARG),
             ("a0_lo on a 3x3", line(1, 8, 8, 8, 8, 64, 0, 9, 1, 0, 0, 128, mask("a0_lo")), CS_E_ARG),
             ("GEGLU at N = 384", line(1, 64, 1, 64, 1, 64, 0, 1, 1, 0, 0, 384, mask(), geglu=1), CS_E_SHAPE),
             ("GEGLU at N = 320 without the 320-column kernels", line(1, 64, 1, 64, 1, 64, 0, 1, 1, 0, 0, 320, mask(), geglu=1, knobs=(("gemm_big", 0),)), CS_E_SHAPE),
             ("no weights", line(1, 8, 8, 8, 8, 64, 0, 9, 1, 0, 0, 128, mask() & ~2), CS_E_ARG),
             ("negative batch", line(-1, 8, 8, 8, 8, 64, 0, 9, 1, 0, 0, 128, mask()), CS_E_SHAPE)]
    got = harness([c[1] for c in cases])
    for (what, ln, code), g in zip(cases, got):
        assert g["rc"] == code and g["family"] == 0, (what, g)
        check_invariants(ln, g)
    # an empty shape is no error and launches nothing; GEGLU at N = 320 is routed to the 320-column kernels under the default knobs
    empty, geglu = harness([line(0, 8, 8, 8, 8, 64, 0, 9, 1, 0, 0, 128, mask()), line(1, 64, 1, 64, 1, 64, 0, 1, 1, 0, 0, 320, mask(), geglu=1)])
    assert empty["rc"] == CS_OK and empty["family"] == 0 and empty["grid_x"] == 0
    assert geglu["rc"] == CS_OK and FAMILIES[geglu["family"]] == "gemm_w8" and geglu["variant"] == 1


# where  B Hi Wi Ho Wo c0 c1 taps stride upsample pad_after_only N geglu lo8 ln_groups pointer_mask splitk_ws_bytes -> family tile_cols variant splits gn_done row_groups
SD15_ROUTES = """
unet_b2  1 128 1 128 1 1280 0 1 1 0 0 10240 1 0 1 376839 33554432 -> 1 128 17 1 0 0
unet_b2  1 128 1 128 1 1280 0 1 1 0 0 1280 0 0 1 376839 33554432 -> 1 128 0 2 0 0
unet_b2  1 128 1 128 1 1280 0 1 1 0 0 1280 0 1 0 268759 33554432 -> 1 128 0 2 0 0
unet_b2  1 128 1 128 1 1280 0 1 1 0 0 3840 0 0 1 376839 33554432 -> 1 128 0 2 0 0
unet_b2  1 128 1 128 1 5120 0 1 1 0 0 1280 0 1 0 262359 33554432 -> 1 128 0 8 0 0
unet_b2  1 154 1 154 1 768 0 1 1 0 0 1280 0 0 0 262151 33554432 -> 1 128 0 1 0 0
unet_b2  1 154 1 154 1 768 0 1 1 0 0 2560 0 0 0 262151 33554432 -> 1 128 0 1 0 0
unet_b2  1 154 1 154 1 768 0 1 1 0 0 640 0 0 0 262151 33554432 -> 1 128 0 1 0 0
unet_b2  1 2048 1 2048 1 2560 0 1 1 0 0 640 0 1 0 262359 33554432 -> 1 128 0 4 0 0
unet_b2  1 2048 1 2048 1 640 0 1 1 0 0 1920 0 0 10 376839 33554432 -> 1 128 1 1 0 0
unet_b2  1 2048 1 2048 1 640 0 1 1 0 0 5120 1 0 10 376839 33554432 -> 1 128 17 1 0 0
unet_b2  1 2048 1 2048 1 640 0 1 1 0 0 640 0 0 10 376839 33554432 -> 1 128 1 1 0 0
unet_b2  1 2048 1 2048 1 640 0 1 1 0 0 640 0 1 0 268759 33554432 -> 1 128 6 1 0 10
unet_b2  1 512 1 512 1 1280 0 1 1 0 0 10240 1 0 1 376839 33554432 -> 1 128 17 1 0 0
unet_b2  1 512 1 512 1 1280 0 1 1 0 0 1280 0 0 1 376839 33554432 -> 1 128 0 2 0 0
unet_b2  1 512 1 512 1 1280 0 1 1 0 0 1280 0 1 0 268759 33554432 -> 1 128 0 2 0 0
unet_b2  1 512 1 512 1 1280 0 1 1 0 0 3840 0 0 1 376839 33554432 -> 1 128 0 2 0 0
unet_b2  1 512 1 512 1 5120 0 1 1 0 0 1280 0 1 0 262359 33554432 -> 1 128 0 8 0 0
unet_b2  1 8192 1 8192 1 1280 0 1 1 0 0 320 0 1 0 262359 33554432 -> 1 160 0 2 0 0
unet_b2  1 8192 1 8192 1 320 0 1 1 0 0 2560 1 0 1 376839 33554432 -> 6 320 3 1 0 0
unet_b2  1 8192 1 8192 1 320 0 1 1 0 0 320 0 1 0 268759 33554432 -> 1 160 6 1 0 4
unet_b2  1 8192 1 8192 1 320 0 1 1 0 0 960 0 0 4 376839 33554432 -> 7 160 1 1 0 0
unet_b2  2 16 16 16 16 1280 0 1 1 0 0 1280 0 0 0 270807 33554432 -> 1 128 0 2 0 0
unet_b2  2 16 16 16 16 1280 0 1 1 0 0 1280 0 1 0 268567 33554432 -> 1 128 0 2 0 0
unet_b2  2 16 16 16 16 1280 0 9 1 0 0 1280 0 0 0 270391 33554432 -> 1 128 32 4 0 0
unet_b2  2 16 16 16 16 1280 0 9 1 0 0 1280 0 0 0 270807 33554432 -> 1 128 32 4 0 0
unet_b2  2 16 16 16 16 1280 1280 1 1 0 0 1280 0 0 0 263967 33554432 -> 1 128 0 8 0 0
unet_b2  2 16 16 16 16 1280 640 1 1 0 0 1280 0 0 0 263967 33554432 -> 1 128 0 4 0 0
unet_b2  2 16 16 16 16 1920 0 9 1 0 0 1280 0 0 0 270391 33554432 -> 1 128 32 2 0 0
unet_b2  2 16 16 16 16 2560 0 9 1 0 0 1280 0 0 0 270391 33554432 -> 1 128 32 8 0 0
unet_b2  2 16 16 16 16 640 0 1 1 0 0 1280 0 0 0 262935 33554432 -> 1 128 0 2 0 0
unet_b2  2 16 16 16 16 640 0 9 1 0 0 1280 0 0 0 270391 33554432 -> 1 128 32 2 0 0
unet_b2  2 16 16 32 32 1280 0 9 1 1 0 1280 0 0 0 270615 33554432 -> 1 128 32 2 0 0
unet_b2  2 16 16 8 8 1280 0 9 2 0 0 1280 0 0 0 270615 33554432 -> 1 128 32 4 1 0
unet_b2  2 32 32 16 16 640 0 9 2 0 0 640 0 0 0 270615 33554432 -> 1 128 32 2 0 0
unet_b2  2 32 32 32 32 1280 0 9 1 0 0 640 0 0 0 270391 33554432 -> 1 128 32 4 0 0
unet_b2  2 32 32 32 32 1280 640 1 1 0 0 640 0 0 0 263967 33554432 -> 1 128 0 4 0 0
unet_b2  2 32 32 32 32 1920 0 9 1 0 0 640 0 0 0 270391 33554432 -> 1 128 32 2 0 0
unet_b2  2 32 32 32 32 320 0 1 1 0 0 640 0 0 0 262935 33554432 -> 1 128 0 1 0 0
unet_b2  2 32 32 32 32 320 0 9 1 0 0 640 0 0 0 270391 33554432 -> 1 128 32 1 1 0
unet_b2  2 32 32 32 32 640 0 1 1 0 0 640 0 0 0 270807 33554432 -> 1 128 0 1 1 0
unet_b2  2 32 32 32 32 640 0 1 1 0 0 640 0 1 0 268567 33554432 -> 1 128 6 1 0 10
unet_b2  2 32 32 32 32 640 0 9 1 0 0 640 0 0 0 270391 33554432 -> 1 128 32 2 0 0
unet_b2  2 32 32 32 32 640 0 9 1 0 0 640 0 0 0 270807 33554432 -> 1 128 32 2 0 0
unet_b2  2 32 32 32 32 640 320 1 1 0 0 640 0 0 0 263967 33554432 -> 1 128 0 2 0 0
unet_b2  2 32 32 32 32 640 640 1 1 0 0 640 0 0 0 263967 33554432 -> 1 128 0 4 0 0
unet_b2  2 32 32 32 32 960 0 9 1 0 0 640 0 0 0 270391 33554432 -> 1 128 32 1 1 0
unet_b2  2 32 32 64 64 640 0 9 1 1 0 640 0 0 0 270615 33554432 -> 1 128 32 1 1 0
unet_b2  2 64 64 32 32 320 0 9 2 0 0 320 0 0 0 270615 33554432 -> 1 160 32 1 1 0
unet_b2  2 64 64 64 64 320 0 1 1 0 0 320 0 0 0 270807 33554432 -> 1 160 0 1 1 0
unet_b2  2 64 64 64 64 320 0 1 1 0 0 320 0 1 0 268567 33554432 -> 1 160 6 1 0 4
unet_b2  2 64 64 64 64 320 0 9 1 0 0 320 0 0 0 270391 33554432 -> 1 160 32 1 1 0
unet_b2  2 64 64 64 64 320 0 9 1 0 0 320 0 0 0 270807 33554432 -> 1 160 32 1 1 0
unet_b2  2 64 64 64 64 320 320 1 1 0 0 320 0 0 0 263967 33554432 -> 1 160 0 2 0 0
unet_b2  2 64 64 64 64 64 0 9 1 0 0 320 0 0 0 270615 33554432 -> 1 160 32 1 1 0
unet_b2  2 64 64 64 64 640 0 9 1 0 0 320 0 0 0 270391 33554432 -> 1 160 32 2 0 0
unet_b2  2 64 64 64 64 640 320 1 1 0 0 320 0 0 0 263967 33554432 -> 1 160 0 2 0 0
unet_b2  2 64 64 64 64 960 0 9 1 0 0 320 0 0 0 270391 33554432 -> 1 160 32 1 1 0
unet_b2  2 8 8 16 16 1280 0 9 1 1 0 1280 0 0 0 270615 33554432 -> 1 128 32 4 0 0
unet_b2  2 8 8 8 8 1280 0 1 1 0 0 1280 0 0 0 270807 33554432 -> 1 128 0 2 1 0
unet_b2  2 8 8 8 8 1280 0 1 1 0 0 1280 0 1 0 268567 33554432 -> 1 128 0 2 0 0
unet_b2  2 8 8 8 8 1280 0 9 1 0 0 1280 0 0 0 270391 33554432 -> 1 128 32 4 1 0
unet_b2  2 8 8 8 8 1280 0 9 1 0 0 1280 0 0 0 270807 33554432 -> 1 128 32 4 1 0
unet_b2  2 8 8 8 8 1280 1280 1 1 0 0 1280 0 0 0 263967 33554432 -> 1 128 0 8 0 0
unet_b2  2 8 8 8 8 2560 0 9 1 0 0 1280 0 0 0 270391 33554432 -> 1 128 32 8 1 0
unet_b32 1 131072 1 131072 1 1280 0 1 1 0 0 320 0 1 0 262359 285212672 -> 6 320 5 1 0 0
unet_b32 1 131072 1 131072 1 320 0 1 1 0 0 2560 1 0 1 376839 285212672 -> 8 32 3 1 0 0
unet_b32 1 131072 1 131072 1 320 0 1 1 0 0 320 0 1 0 268759 285212672 -> 6 320 6 1 0 2
unet_b32 1 131072 1 131072 1 320 0 1 1 0 0 960 0 0 2 376839 285212672 -> 8 32 2 1 0 0
unet_b32 1 2048 1 2048 1 1280 0 1 1 0 0 10240 1 0 1 376839 285212672 -> 6 320 3 1 0 0
unet_b32 1 2048 1 2048 1 1280 0 1 1 0 0 1280 0 0 1 376839 285212672 -> 1 128 0 2 0 0
unet_b32 1 2048 1 2048 1 1280 0 1 1 0 0 1280 0 1 0 268759 285212672 -> 1 128 0 2 0 0
unet_b32 1 2048 1 2048 1 1280 0 1 1 0 0 3840 0 0 1 376839 285212672 -> 7 160 1 1 0 0
unet_b32 1 2048 1 2048 1 5120 0 1 1 0 0 1280 0 1 0 262359 285212672 -> 1 128 0 2 0 0
unet_b32 1 2464 1 2464 1 768 0 1 1 0 0 1280 0 0 0 262151 285212672 -> 1 128 0 1 0 0
unet_b32 1 2464 1 2464 1 768 0 1 1 0 0 2560 0 0 0 262151 285212672 -> 1 128 0 1 0 0
unet_b32 1 2464 1 2464 1 768 0 1 1 0 0 640 0 0 0 262151 285212672 -> 1 128 0 1 0 0
unet_b32 1 32768 1 32768 1 2560 0 1 1 0 0 640 0 1 0 262359 285212672 -> 6 320 5 1 0 0
unet_b32 1 32768 1 32768 1 640 0 1 1 0 0 1920 0 0 4 376839 285212672 -> 6 320 2 1 0 0
unet_b32 1 32768 1 32768 1 640 0 1 1 0 0 5120 1 0 4 376839 285212672 -> 6 320 3 1 0 0
unet_b32 1 32768 1 32768 1 640 0 1 1 0 0 640 0 0 4 376839 285212672 -> 6 320 2 1 0 0
unet_b32 1 32768 1 32768 1 640 0 1 1 0 0 640 0 1 0 268759 285212672 -> 6 320 6 1 0 4
unet_b32 1 8192 1 8192 1 1280 0 1 1 0 0 10240 1 0 8 376839 285212672 -> 6 320 3 1 0 0
unet_b32 1 8192 1 8192 1 1280 0 1 1 0 0 1280 0 0 8 376839 285212672 -> 7 160 1 1 0 0
unet_b32 1 8192 1 8192 1 1280 0 1 1 0 0 1280 0 1 0 268759 285212672 -> 7 160 4 1 0 8
unet_b32 1 8192 1 8192 1 1280 0 1 1 0 0 3840 0 0 8 376839 285212672 -> 6 320 2 1 0 0
unet_b32 1 8192 1 8192 1 5120 0 1 1 0 0 1280 0 1 0 262359 285212672 -> 7 160 3 1 0 0
unet_b32 32 16 16 16 16 1280 0 1 1 0 0 1280 0 0 0 270807 285212672 -> 7 160 0 1 1 0
unet_b32 32 16 16 16 16 1280 0 1 1 0 0 1280 0 1 0 268567 285212672 -> 7 160 4 1 0 8
unet_b32 32 16 16 16 16 1280 0 9 1 0 0 1280 0 0 0 270391 285212672 -> 3 160 0 1 1 0
unet_b32 32 16 16 16 16 1280 0 9 1 0 0 1280 0 0 0 270807 285212672 -> 3 160 0 1 1 0
unet_b32 32 16 16 16 16 1280 1280 1 1 0 0 1280 0 0 0 263967 285212672 -> 7 160 0 1 0 0
unet_b32 32 16 16 16 16 1280 640 1 1 0 0 1280 0 0 0 263967 285212672 -> 7 160 0 1 0 0
unet_b32 32 16 16 16 16 1920 0 9 1 0 0 1280 0 0 0 270391 285212672 -> 3 160 0 1 1 0
unet_b32 32 16 16 16 16 2560 0 9 1 0 0 1280 0 0 0 270391 285212672 -> 3 160 0 1 1 0
unet_b32 32 16 16 16 16 640 0 1 1 0 0 1280 0 0 0 262935 285212672 -> 7 160 0 1 0 0
unet_b32 32 16 16 16 16 640 0 9 1 0 0 1280 0 0 0 270391 285212672 -> 3 160 0 1 1 0
unet_b32 32 16 16 32 32 1280 0 9 1 1 0 1280 0 0 0 270615 285212672 -> 3 160 5 1 1 0
unet_b32 32 16 16 8 8 1280 0 9 2 0 0 1280 0 0 0 270615 285212672 -> 1 128 32 2 1 0
unet_b32 32 32 32 16 16 640 0 9 2 0 0 640 0 0 0 270615 285212672 -> 1 128 32 1 1 0
unet_b32 32 32 32 32 32 1280 0 9 1 0 0 640 0 0 0 270391 285212672 -> 3 160 0 1 1 0
unet_b32 32 32 32 32 32 1280 640 1 1 0 0 640 0 0 0 263967 285212672 -> 6 320 0 1 0 0
unet_b32 32 32 32 32 32 1920 0 9 1 0 0 640 0 0 0 270391 285212672 -> 3 160 0 1 1 0
unet_b32 32 32 32 32 32 320 0 1 1 0 0 640 0 0 0 262935 285212672 -> 6 320 0 1 0 0
unet_b32 32 32 32 32 32 320 0 9 1 0 0 640 0 0 0 270391 285212672 -> 3 160 0 1 1 0
unet_b32 32 32 32 32 32 640 0 1 1 0 0 640 0 0 0 270807 285212672 -> 6 320 0 1 1 0
unet_b32 32 32 32 32 32 640 0 1 1 0 0 640 0 1 0 268567 285212672 -> 6 320 6 1 0 4
unet_b32 32 32 32 32 32 640 0 9 1 0 0 640 0 0 0 270391 285212672 -> 3 160 0 1 1 0
unet_b32 32 32 32 32 32 640 0 9 1 0 0 640 0 0 0 270807 285212672 -> 3 160 0 1 1 0
unet_b32 32 32 32 32 32 640 320 1 1 0 0 640 0 0 0 263967 285212672 -> 6 320 0 1 0 0
unet_b32 32 32 32 32 32 640 640 1 1 0 0 640 0 0 0 263967 285212672 -> 6 320 0 1 0 0
unet_b32 32 32 32 32 32 960 0 9 1 0 0 640 0 0 0 270391 285212672 -> 3 160 0 1 1 0
unet_b32 32 32 32 64 64 640 0 9 1 1 0 640 0 0 0 270615 285212672 -> 3 160 5 1 1 0
unet_b32 32 64 64 32 32 320 0 9 2 0 0 320 0 0 0 270615 285212672 -> 1 160 32 1 1 0
unet_b32 32 64 64 64 64 320 0 1 1 0 0 320 0 0 0 270807 285212672 -> 6 320 0 1 1 0
unet_b32 32 64 64 64 64 320 0 1 1 0 0 320 0 1 0 268567 285212672 -> 6 320 6 1 0 2
unet_b32 32 64 64 64 64 320 0 9 1 0 0 320 0 0 0 270391 285212672 -> 3 160 0 1 1 0
unet_b32 32 64 64 64 64 320 0 9 1 0 0 320 0 0 0 270807 285212672 -> 3 160 0 1 1 0
unet_b32 32 64 64 64 64 320 320 1 1 0 0 320 0 0 0 263967 285212672 -> 6 320 0 1 0 0
unet_b32 32 64 64 64 64 64 0 9 1 0 0 320 0 0 0 270615 285212672 -> 3 160 0 1 1 0
unet_b32 32 64 64 64 64 640 0 9 1 0 0 320 0 0 0 270391 285212672 -> 3 160 0 1 1 0
unet_b32 32 64 64 64 64 640 320 1 1 0 0 320 0 0 0 263967 285212672 -> 6 320 0 1 0 0
unet_b32 32 64 64 64 64 960 0 9 1 0 0 320 0 0 0 270391 285212672 -> 3 160 0 1 1 0
unet_b32 32 8 8 16 16 1280 0 9 1 1 0 1280 0 0 0 270615 285212672 -> 3 160 5 1 1 0
unet_b32 32 8 8 8 8 1280 0 1 1 0 0 1280 0 0 0 270807 285212672 -> 1 128 0 2 1 0
unet_b32 32 8 8 8 8 1280 0 1 1 0 0 1280 0 1 0 268567 285212672 -> 1 128 0 2 0 0
unet_b32 32 8 8 8 8 1280 0 9 1 0 0 1280 0 0 0 270391 285212672 -> 3 160 10 4 1 0
unet_b32 32 8 8 8 8 1280 0 9 1 0 0 1280 0 0 0 270807 285212672 -> 3 160 10 4 1 0
unet_b32 32 8 8 8 8 1280 1280 1 1 0 0 1280 0 0 0 263967 285212672 -> 1 128 0 2 0 0
unet_b32 32 8 8 8 8 2560 0 9 1 0 0 1280 0 0 0 270391 285212672 -> 3 160 10 4 1 0
vae_dec  1 128 128 128 128 512 0 9 1 0 0 512 0 0 0 8215 0 -> 3 128 6 1 1 0
vae_dec  1 128 128 128 128 512 0 9 1 0 0 512 0 0 0 8279 0 -> 3 128 6 1 1 0
vae_dec  1 128 128 256 256 512 0 9 1 1 0 512 0 0 0 139287 0 -> 4 128 2 1 1 0
vae_dec  1 256 256 256 256 256 0 9 1 0 0 256 0 0 0 8215 0 -> 3 128 6 1 1 0
vae_dec  1 256 256 256 256 256 0 9 1 0 0 256 0 0 0 8279 0 -> 3 128 6 1 1 0
vae_dec  1 256 256 256 256 512 0 1 1 0 0 256 0 0 0 23 0 -> 1 128 0 1 0 0
vae_dec  1 256 256 256 256 512 0 9 1 0 0 256 0 0 0 8215 0 -> 3 128 6 1 1 0
vae_dec  1 256 256 512 512 256 0 9 1 1 0 256 0 0 0 139287 0 -> 4 128 2 1 1 0
vae_dec  1 4096 1 4096 1 4096 0 1 1 0 0 512 0 0 0 23 0 -> 1 128 0 1 0 0
vae_dec  1 4096 1 4096 1 512 0 1 1 0 0 4096 0 0 0 7 0 -> 1 128 0 1 0 0
vae_dec  1 4096 1 4096 1 512 0 1 1 0 0 512 0 0 0 23 0 -> 1 128 0 1 0 0
vae_dec  1 4096 1 4096 1 512 0 1 1 0 0 512 0 0 0 87 0 -> 1 128 0 1 0 0
vae_dec  1 512 1 512 1 512 0 1 1 0 0 4096 0 0 0 7 0 -> 1 128 0 1 0 0
vae_dec  1 512 512 512 512 128 0 9 1 0 0 128 0 0 0 8215 0 -> 3 128 6 1 1 0
vae_dec  1 512 512 512 512 128 0 9 1 0 0 128 0 0 0 8279 0 -> 3 128 6 1 1 0
vae_dec  1 512 512 512 512 256 0 1 1 0 0 128 0 0 0 23 0 -> 1 128 0 1 0 0
vae_dec  1 512 512 512 512 256 0 9 1 0 0 128 0 0 0 8215 0 -> 3 128 6 1 1 0
vae_dec  1 64 64 128 128 512 0 9 1 1 0 512 0 0 0 139287 0 -> 4 128 2 1 1 0
vae_dec  1 64 64 64 64 512 0 9 1 0 0 512 0 0 0 8215 0 -> 1 128 32 1 1 0
vae_dec  1 64 64 64 64 512 0 9 1 0 0 512 0 0 0 8279 0 -> 1 128 32 1 1 0
"""


def test_sd15_unet_and_vae_decoder_layers_keep_their_routes(harness):
    rows = [r.split("->") for r in SD15_ROUTES.strip().splitlines()]
    lines = [" ".join(r[0].split()[1:]) for r in rows]
    assert len(lines) == 150 and len(set(lines)) == 150
    seen = set()
    for (head, want), ln, got in zip(rows, lines, harness(lines)):
        fam, cols, variant, splits, gn_done, row_groups = (int(x) for x in want.split())
        expect_route(head.strip(), got, fam, cols, variant, splits, gn_done, row_groups)
        check_invariants(ln, got)
        seen.add(FAMILIES[fam])
    assert seen == {"generic", "conv3_lw", "sub_pixel", "gemm_w8", "gemm_lw", "gemm_as"}      # what the flagship models run on under the default knobs
