"""The C-ABI library loads (no GPU needed) and exports every symbol include/pegasus_raster.h declares;
argument validation works without touching a device."""
import ctypes as C
import re
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]


def declared_symbols():
    text = (ROOT / "include" / "pegasus_raster.h").read_text()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(pgr_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    from pegasus_amd import _lib
    from pegasus_amd import build
    build.build()
    lib = _lib.lib()
    names = declared_symbols()
    assert len(names) >= 12
    for name in names:
        assert hasattr(lib, name), f"{name} declared in include/pegasus_raster.h but not exported"
        assert name in _lib.SYMBOLS, f"{name} has no ctypes prototype in pegasus_amd/_lib.py"
    assert set(_lib.SYMBOLS) == set(names)


def test_version_and_status_strings():
    from pegasus_amd import _lib
    lib = _lib.lib()
    assert lib.pgr_abi_version() == 4 == _lib.PGR_ABI_VERSION
    assert b"gfx950" in lib.pgr_version()
    assert lib.pgr_status_string(0) == b"ok"
    assert lib.pgr_status_string(-3) == b"instance buffer overflow"


def test_workspace_sizes_are_host_only():
    from pegasus_amd import _lib
    lib = _lib.lib()
    one = lib.pgr_workspace_bytes(100_000, 800, 800, 1 << 20)
    assert one > 100_000 * 56 + (1 << 20) * 20
    assert lib.pgr_batch_workspace_bytes(100_000, 800, 800, 1 << 20, 8) > 7 * one
    assert lib.pgr_workspace_bytes(-1, 800, 800, 10) == 0
    assert lib.pgr_workspace_bytes(10, 0, 800, 10) == 0


def test_frame_record_layout_is_host_only_and_aligned():
    from pegasus_amd import _lib, masks as M
    lay = M.record_layout(800, 800, 8)
    assert lay == dict(off_rgb=0, off_depth=1_920_000, off_masks=3_200_000, bytes=3_840_000)      # 3.84 MB
    odd = M.record_layout(5, 7, 11)
    assert all(v % 16 == 0 for v in odd.values()) and odd["off_depth"] >= 105 and odd["off_masks"] >= odd["off_depth"] + 70
    assert odd["bytes"] >= odd["off_masks"] + 2 * 35
    assert _lib.lib().pgr_frame_record_layout(0, 5, 1, None) == _lib.PGR_ERR_INVALID_ARGUMENT
    assert _lib.lib().pgr_scene_cache_bytes(1000) >= 5000 and _lib.lib().pgr_scene_cache_bytes(-1) == 0
    assert _lib.lib().pgr_layers_workspace_bytes(1000, 64, 64, 1 << 16, 2, 8) > _lib.lib().pgr_batch_workspace_bytes(1000, 64, 64, 1 << 16, 2)
    assert _lib.lib().pgr_layers_workspace_bytes(1000, 64, 64, 1 << 16, 2, 0) == 0


def test_invalid_arguments_are_rejected_before_any_launch():
    from pegasus_amd import _lib
    lib = _lib.lib()
    scene = _lib.PgrScene(n=10)             # no pointers
    cam = _lib.PgrCamera(image_width=64, image_height=64, tanfovx=0.5, tanfovy=0.5)
    out = _lib.PgrOutputs()
    need = C.c_int64(0)
    rc = lib.pgr_forward(_forward_call(_lib, scene, cam, out, num_instances=C.pointer(need)), None)
    assert rc == _lib.PGR_ERR_INVALID_ARGUMENT
    with pytest.raises(ValueError):
        _lib.check(rc, "pgr_forward")
    assert lib.pgr_mark_visible(-1, None, None, None, None) == _lib.PGR_ERR_INVALID_ARGUMENT
    assert lib.pgr_color_masks(None, 1, 8, 8, None, 1, 0.1, None, None) == _lib.PGR_ERR_INVALID_ARGUMENT


def _forward_call(_lib, scene, cam, out, workspace=None, workspace_bytes=0, **fields):
    """A one-view PgrForwardCall at capacity 100; ``fields`` sets or overrides anything."""
    kw = dict(scene=C.pointer(scene), n_views=1, cameras=C.pointer(cam), outs=C.pointer(out), workspace=workspace,
              workspace_bytes=workspace_bytes, max_instances_per_view=100)
    kw.update(fields)
    return _lib.PgrForwardCall(**kw)


def test_rasterizer_refuses_cpu_tensors():
    import torch
    from pegasus_amd import diff_gaussian_rasterization as dgr
    s = dgr.GaussianRasterizationSettings(8, 8, 0.5, 0.5, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0,
                                          torch.zeros(3), False, False)
    r = dgr.GaussianRasterizer(s)
    with pytest.raises(RuntimeError, match="no CPU path"):
        r(torch.zeros(4, 3), None, torch.zeros(4, 1), shs=torch.zeros(4, 16, 3), scales=torch.ones(4, 3),
          rotations=torch.zeros(4, 4))
    with pytest.raises(Exception, match="excatly one of either SHs or precomputed colors"):
        r(torch.zeros(4, 3), None, torch.zeros(4, 1), scales=torch.ones(4, 3), rotations=torch.zeros(4, 4))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(torch.zeros(4, 3), None, torch.zeros(4, 1), shs=torch.zeros(4, 16, 3), scales=torch.ones(4, 3))


def test_new_entry_points_validate_before_any_launch():
    """PgrForwardCall.layers / sem_masks / depth_mode / pgr_pack_records / pgr_scene_prepare: argument misuse is an
    integer status from host-side checks (fake non-NULL device pointers are never dereferenced; no device is touched)."""
    from pegasus_amd import _lib
    lib = _lib.lib()
    fake = C.c_void_p(0x1000)
    scene = _lib.PgrScene(n=10, means3d=fake, opacities=fake, scales=fake, rotations=fake, shs=fake, sh_degree=0, sh_stride=1,
                          scale_modifier=1.0)
    cam = _lib.PgrCamera(image_width=64, image_height=64, tanfovx=0.5, tanfovy=0.5, viewmatrix=fake, projmatrix=fake,
                         campos=fake, bg=fake, depth_mode=0)
    scratch = (C.c_char * int(lib.pgr_host_scratch_bytes(1)))()
    good_layers = _lib.PgrLayers(layer_id=fake, n_layers=3, mask_colors=fake, mask_threshold=0.1)

    host = dict(host_scratch=C.addressof(scratch), host_scratch_bytes=len(scratch))

    def layers_rc(layers, out, camera=cam):
        return lib.pgr_forward(_forward_call(_lib, scene, camera, out, layers=None if layers is None else C.pointer(layers),
                                             **host), None)
    no_masks = _lib.PgrOutputs(color=fake, depth=fake)
    with_masks = _lib.PgrOutputs(sem_masks=fake)
    assert layers_rc(None, with_masks) == _lib.PGR_ERR_INVALID_ARGUMENT                       # no descriptor
    assert layers_rc(good_layers, no_masks) == _lib.PGR_ERR_INVALID_ARGUMENT                  # a layered call's one output
    for bad in (_lib.PgrLayers(layer_id=None, n_layers=3, mask_colors=fake), _lib.PgrLayers(layer_id=fake, n_layers=0, mask_colors=fake),
                _lib.PgrLayers(layer_id=fake, n_layers=3, mask_colors=None), _lib.PgrLayers(layer_id=fake, n_layers=5000, mask_colors=fake)):
        assert layers_rc(bad, with_masks) == _lib.PGR_ERR_INVALID_ARGUMENT
    # everything valid but the workspace: the checks got that far without touching a device
    assert layers_rc(good_layers, with_masks) == _lib.PGR_ERR_INVALID_ARGUMENT                # workspace == NULL
    # depth_mode outside the enum
    bad_cam = _lib.PgrCamera(image_width=64, image_height=64, tanfovx=0.5, tanfovy=0.5, viewmatrix=fake, projmatrix=fake,
                             campos=fake, bg=fake, depth_mode=7)
    need = C.c_int64(0)
    out = _lib.PgrOutputs(color=fake, depth=fake, radii=fake)
    assert lib.pgr_forward(_forward_call(_lib, scene, bad_cam, out, num_instances=C.pointer(need)), None) == _lib.PGR_ERR_INVALID_ARGUMENT
    # masks from the compositor's epilogue need the colours to threshold against
    sem = _lib.PgrSemantic(object_id=fake, colors=fake, n_env=5, k_objects=2)                 # no mask_colors
    out_m = _lib.PgrOutputs(color=fake, depth=fake, sem_color=fake, sem_masks=fake)
    assert lib.pgr_forward(_forward_call(_lib, scene, cam, out_m, semantic=C.pointer(sem), **host), None) == _lib.PGR_ERR_INVALID_ARGUMENT
    # the split SH layout (PgrScene::shs_rest): needs the first coefficient in `shs` and room for more than one; the
    # backward takes the concatenated layout only (its SH gradient is one array)
    for bad_scene in (_lib.PgrScene(n=10, means3d=fake, opacities=fake, scales=fake, rotations=fake, colors_precomp=fake,
                                    shs_rest=fake, scale_modifier=1.0),
                      _lib.PgrScene(n=10, means3d=fake, opacities=fake, scales=fake, rotations=fake, shs=fake, shs_rest=fake,
                                    sh_degree=0, sh_stride=1, scale_modifier=1.0)):
        assert lib.pgr_forward(_forward_call(_lib, bad_scene, cam, out, num_instances=C.pointer(need)), None) == _lib.PGR_ERR_INVALID_ARGUMENT
    split = _lib.PgrScene(n=10, means3d=fake, opacities=fake, scales=fake, rotations=fake, shs=fake, shs_rest=fake, sh_degree=3,
                          sh_stride=16, scale_modifier=1.0)
    posed = _lib.PgrPosedObjects(object_id=fake, poses=fake, k_objects=2)
    assert lib.pgr_forward(_forward_call(_lib, split, cam, out, fake, 1 << 30, posed=C.pointer(posed), **host),
                           None) == _lib.PGR_ERR_INVALID_ARGUMENT
    grads = _lib.PgrGradOutputs()
    view = _lib.PgrBackwardView(grad_color=fake, final_T=fake, n_contrib=fake, radii=fake)
    back = _lib.PgrBackwardCall(scene=C.pointer(split), n_views=1, cameras=C.pointer(cam), views=C.pointer(view), workspace=fake,
                                workspace_bytes=1 << 30, max_instances_per_view=100, grads=C.pointer(grads), scratch=fake,
                                scratch_bytes=lib.pgr_backward_batch_scratch_bytes(10, 1))
    assert lib.pgr_backward(back, None) == _lib.PGR_ERR_INVALID_ARGUMENT
    # records: stride below the layout's size, unaligned stride, NULL destination
    lay = _lib.PgrRecordLayout()
    assert lib.pgr_frame_record_layout(16, 16, 8, C.byref(lay)) == 0
    assert lib.pgr_pack_records(fake, fake, fake, 1, 8, 16, 16, fake, lay.bytes - 16, None) == _lib.PGR_ERR_INVALID_ARGUMENT
    assert lib.pgr_pack_records(fake, fake, fake, 1, 8, 16, 16, fake, lay.bytes + 8, None) == _lib.PGR_ERR_INVALID_ARGUMENT
    assert lib.pgr_pack_records(fake, fake, fake, 1, 8, 16, 16, None, lay.bytes, None) == _lib.PGR_ERR_INVALID_ARGUMENT
    assert lib.pgr_pack_records(fake, fake, fake, 0, 8, 16, 16, fake, lay.bytes, None) == 0     # nothing to do
    # scene_prepare: cache too small / missing out-pointers
    p1, p2 = C.c_void_p(), C.c_void_p()
    sc = _lib.PgrScene(n=1000, tie_index=fake)
    assert lib.pgr_scene_prepare(C.byref(sc), None, fake, 16, C.byref(p1), C.byref(p2), None) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL
    assert lib.pgr_scene_prepare(C.byref(sc), None, fake, 1 << 20, None, C.byref(p2), None) == _lib.PGR_ERR_INVALID_ARGUMENT
    empty = _lib.PgrScene(n=0)
    assert lib.pgr_scene_prepare(C.byref(empty), None, None, 0, C.byref(p1), C.byref(p2), None) == 0 and not p1.value and not p2.value


def test_forward_call_rejects_mixed_modes_before_any_launch():
    """What goes with a synchronous call only, with an asynchronous one only, or with neither: PGR_ERR_INVALID_ARGUMENT from
    the host-side checks, with fake pointers and no device.  Every call here has a workspace that is merely too small -- the
    last check before the first enqueue -- so a case let through would answer PGR_ERR_WORKSPACE_TOO_SMALL, as the unmixed
    control calls at the end do: the rejection is the combination's."""
    from pegasus_amd import _lib
    lib = _lib.lib()
    bad, fake = _lib.PGR_ERR_INVALID_ARGUMENT, C.c_void_p(0x1000)
    assert lib.pgr_forward(None, None) == bad                                                  # no call
    scene = _lib.PgrScene(n=10, means3d=fake, opacities=fake, scales=fake, rotations=fake, shs=fake, sh_degree=0, sh_stride=1,
                          scale_modifier=1.0)
    cam = _lib.PgrCamera(image_width=64, image_height=64, tanfovx=0.5, tanfovy=0.5, viewmatrix=fake, projmatrix=fake,
                         campos=fake, bg=fake, depth_mode=0)
    out, out_masks = _lib.PgrOutputs(color=fake, depth=fake, radii=fake), _lib.PgrOutputs(sem_masks=fake)
    scratch = (C.c_char * int(lib.pgr_host_scratch_bytes(1)))()
    host = dict(host_scratch=C.addressof(scratch), host_scratch_bytes=len(scratch))
    posed = C.pointer(_lib.PgrPosedObjects(object_id=fake, poses=fake, k_objects=2))
    layers = C.pointer(_lib.PgrLayers(layer_id=fake, n_layers=3, mask_colors=fake, mask_threshold=0.1))
    need, ms = C.pointer(C.c_int64(0)), (C.c_float * _lib.PGR_NUM_STAGES)()

    def rc(o=out, **fields):
        return lib.pgr_forward(_forward_call(_lib, scene, cam, o, fake, 16, **fields), None)
    # synchronous (no host scratch): no posed objects, no layers, no status event
    assert rc(posed=posed) == bad
    assert rc(o=out_masks, layers=layers) == bad
    assert rc(status_event=fake) == bad
    # asynchronous: no instance counts, no stage times, a host scratch of the full size
    assert rc(num_instances=need, **host) == bad
    assert rc(stage_ms=ms, **host) == bad
    assert rc(host_scratch=C.addressof(scratch), host_scratch_bytes=len(scratch) - 1) == bad
    # the early status words and a layered call do not go together
    assert rc(o=out_masks, layers=layers, status_event=fake, **host) == bad
    # controls: the same fields, unmixed, pass every argument check
    small = _lib.PGR_ERR_WORKSPACE_TOO_SMALL
    assert rc(num_instances=need) == small                      # (stage_ms creates its HIP events first: needs a device)
    assert rc(posed=posed, status_event=fake, **host) == small
    assert rc(o=out_masks, layers=layers, posed=posed, **host) == small


def test_backward_call_rejects_null_and_short_camera_scratch():
    from pegasus_amd import _lib
    lib = _lib.lib()
    bad, fake, n = _lib.PGR_ERR_INVALID_ARGUMENT, C.c_void_p(0x1000), 10
    assert lib.pgr_backward(None, None) == bad
    scene = _lib.PgrScene(n=n, means3d=fake, opacities=fake, scales=fake, rotations=fake, shs=fake, sh_degree=0, sh_stride=1,
                          scale_modifier=1.0)
    cam = _lib.PgrCamera(image_width=64, image_height=48, tanfovx=0.5, tanfovy=0.5)
    view = _lib.PgrBackwardView(grad_color=fake, final_T=fake, n_contrib=fake, radii=fake)
    call = _lib.PgrBackwardCall(scene=C.pointer(scene), n_views=1, cameras=C.pointer(cam), views=C.pointer(view), workspace=fake,
                                workspace_bytes=16, max_instances_per_view=100, grads=C.pointer(_lib.PgrGradOutputs(means3d=fake)),
                                scratch=fake, scratch_bytes=lib.pgr_backward_batch_scratch_bytes(n, 1))
    assert lib.pgr_backward(call, None) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL       # control: every argument check passed
    call.camera_grads = C.pointer(_lib.PgrCameraGrad(viewmatrix=fake))
    assert lib.pgr_backward(call, None) == bad                                     # camera gradients without their scratch
    call.camera_scratch, call.camera_scratch_bytes = fake, lib.pgr_camera_grad_scratch_bytes(n, 1) - 1
    assert lib.pgr_backward(call, None) == bad                                     # one byte short
    call.camera_scratch_bytes += 1
    assert lib.pgr_backward(call, None) == _lib.PGR_ERR_WORKSPACE_TOO_SMALL


def test_stale_or_foreign_library_is_named_not_crashed_on(tmp_path):
    """PGR_LIB pointing at a library of another ABI version (a stale build, a variant built from old sources) or at a
    library that is not this one at all: the loader checks pgr_abi_version FIRST and raises RasterizerLibraryError naming
    the file, instead of an AttributeError on whichever newer entry point the file lacks (round-4 advisor finding)."""
    import subprocess
    import sys
    old = tmp_path / "old.c"
    old.write_text("int pgr_abi_version(void) { return 1; }\nconst char* pgr_version(void) { return \"old\"; }\n")
    foreign = tmp_path / "foreign.c"
    foreign.write_text("int something_else(void) { return 0; }\n")
    for src, needle in ((old, "ABI version 1"), (foreign, "pgr_abi_version")):
        so = src.with_suffix(".so")
        subprocess.run(["gcc", "-shared", "-fPIC", "-o", str(so), str(src)], check=True)
        code = ("import sys; sys.path.insert(0, %r)\n"
                "from pegasus_amd import _lib\n"
                "try:\n    _lib.lib()\nexcept _lib.RasterizerLibraryError as e:\n    print('RLE:', e)\n" % str(ROOT))
        out = subprocess.run([sys.executable, "-c", code], env={**__import__("os").environ, "PGR_LIB": str(so)},
                             capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr
        assert "RLE:" in out.stdout and needle in out.stdout and str(so) in out.stdout, out.stdout + out.stderr


def test_header_is_plain_c_and_the_library_links_from_c(tmp_path):
    """The drop-in boundary is a C ABI: include/pegasus_raster.h compiles as C11 (gcc -std=c11 -Wall -Werror -pedantic) and
    a C program linked against libpegasus_raster.so calls the host-only entry points -- version, status strings, workspace
    sizes, the frame-record layout, and an argument check that returns before any device is touched -- and agrees with the
    ctypes binding.  (The struct sizes it prints are the ones pegasus_amd/_lib.py declares.)"""
    import subprocess
    from pegasus_amd import _lib, build
    build.build()
    src = tmp_path / "abi_probe.c"
    src.write_text(r'''
#include <stdio.h>
#include <stddef.h>
#include "pegasus_raster.h"
int main(void) {
    PgrRecordLayout lay;
    PgrScene scene = {0};
    PgrCamera cam = {0};
    PgrOutputs out = {0};
    PgrForwardCall call = {0};
    int64_t need = -1;
    scene.n = 10;                               /* no pointers: must be rejected on the host */
    cam.image_width = 64; cam.image_height = 64; cam.tanfovx = 0.5f; cam.tanfovy = 0.5f;
    printf("abi %d\n", (int)pgr_abi_version());
    printf("version %s\n", pgr_version());
    printf("status %s\n", pgr_status_string(PGR_ERR_INSTANCE_OVERFLOW));
    printf("ws %zu\n", pgr_batch_workspace_bytes(100000, 800, 800, 1 << 20, 8));
    printf("layout_rc %d\n", (int)pgr_frame_record_layout(800, 800, 8, &lay));
    printf("record %lld %lld %lld\n", (long long)lay.off_depth, (long long)lay.off_masks, (long long)lay.bytes);
    call.scene = &scene; call.n_views = 1; call.cameras = &cam; call.outs = &out;
    call.max_instances_per_view = 100; call.num_instances = &need;
    printf("forward_rc %d\n", (int)pgr_forward(&call, NULL));
    printf("sizes %zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(PgrScene), sizeof(PgrCamera), sizeof(PgrOutputs), sizeof(PgrSemantic),
           sizeof(PgrLayers), sizeof(PgrPosedObjects), sizeof(PgrForwardCall), sizeof(PgrBackwardCall));
    return 0;
}
''')
    exe = tmp_path / "abi_probe"
    lib_dir = str(_lib.LIB_PATH.parent)
    subprocess.run(["gcc", "-std=c11", "-Wall", "-Werror", "-pedantic", f"-I{ROOT / 'include'}", str(src), "-o", str(exe),
                    f"-L{lib_dir}", "-lpegasus_raster", f"-Wl,-rpath,{lib_dir}"], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120, check=True).stdout.splitlines()
    got = dict(l.split(" ", 1) for l in out)
    lib = _lib.lib()
    assert got["abi"] == str(_lib.PGR_ABI_VERSION) and got["version"] == lib.pgr_version().decode()
    assert got["status"] == "instance buffer overflow"
    assert int(got["ws"]) == lib.pgr_batch_workspace_bytes(100000, 800, 800, 1 << 20, 8)
    assert got["layout_rc"] == "0" and got["record"] == "1920000 3200000 3840000"
    assert int(got["forward_rc"]) == _lib.PGR_ERR_INVALID_ARGUMENT
    sizes = [int(x) for x in got["sizes"].split()]
    assert sizes == [C.sizeof(t) for t in (_lib.PgrScene, _lib.PgrCamera, _lib.PgrOutputs, _lib.PgrSemantic, _lib.PgrLayers,
                                           _lib.PgrPosedObjects, _lib.PgrForwardCall, _lib.PgrBackwardCall)]


def test_loading_the_library_leaves_one_hip_runtime_in_the_process():
    """torch's wheel bundles its own libamdhip64 / libhsa-runtime64; the library must bind to THAT runtime whichever of the two
    is asked for first (pegasus_amd._lib.lib() imports torch before dlopen).  With the system runtime loaded beside torch's,
    every HIP call of the library failed with "no ROCm-capable device is detected" (build() then smoke() in one process)."""
    import subprocess
    import sys
    root = str(Path(__file__).resolve().parents[1])
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from pegasus_amd import _lib\n"
            "_lib.lib()\n"
            "import torch\n"
            "maps = open('/proc/self/maps').read()\n"
            "hip = sorted({l.split()[-1] for l in maps.splitlines() if 'libamdhip64' in l})\n"
            "hsa = sorted({l.split()[-1] for l in maps.splitlines() if 'libhsa-runtime64' in l})\n"
            "print(hip, hsa)\n"
            "assert len(hip) == 1 and len(hsa) <= 1, (hip, hsa)\n") % root
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr

