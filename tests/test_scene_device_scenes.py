"""CPU side of the device-resident scene update: the scenes of tests/scene_device_scenes.py do what tests/test_gpu_scene_device.py needs
them to do, and the binding declares the new entry points.  No GPU."""
import numpy as np

import block_scenes as B
import scene_device_scenes as D


def test_the_binding_declares_the_entry_points(pkg):
    assert "vrt_hip_set_gaussians_device" in pkg.SYMBOLS and "vrt_hip_get_ray_index_perm" in pkg.SYMBOLS
    assert len(pkg.SYMBOLS["vrt_hip_set_gaussians_device"][1]) == 7
    assert hasattr(pkg.Renderer, "set_gaussians_device") and hasattr(pkg.Renderer, "ray_index_perm")
    header = open(pkg.INCLUDE_DIR + "/vrt_hip.h").read()
    assert "vrt_hip_set_gaussians_device(" in header and "vrt_hip_get_ray_index_perm(" in header


def test_packed_arrays_are_the_setters_layout(oracle):
    g = D.cloud(oracle, 65)
    mu, alb, sig, mag = D.packed(g)
    assert mu.shape == (65, 3) and alb.shape == (65, 4) and sig.shape == mag.shape == (65,)
    assert all(a.dtype == np.float32 and a.flags.c_contiguous for a in (mu, alb, sig, mag))
    assert (alb[:, 3] == g["albedo"][:, 3]).all() and (mu[:, 2] == g["mu"][:, 2]).all()
    assert all(len(a) == 0 for a in D.packed(D.cloud(oracle, 0)))
    o, d = D.rays()
    assert d.shape == (130, 3) and np.allclose(np.linalg.norm(d.astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_tie_scene_has_equal_keys_across_a_leaf_border(oracle):
    g = D.tie_scene(oracle)
    perm = D.morton_order(g)
    key = D.morton_keys(g)[perm]
    assert key[D.LEAF - 1] == key[D.LEAF]                                   # positions 63 and 64: one key, two leaves
    run = np.flatnonzero(key == key[D.LEAF])
    assert run[0] <= D.LEAF - 4 and run[-1] >= D.LEAF + 3 and len(run) >= 12
    members = perm[run]
    assert (np.diff(members.astype(np.int64)) > 0).all()                    # ties by scene index ...
    assert (np.diff(members.astype(np.int64)) > 1).any()                    # ... of Gaussians scattered over the scene
    assert len(np.unique(key)) > len(g) // 2                                # the rest of the scene is an ordinary cloud


def test_flat_scene_has_an_axis_without_extent(oracle):
    g = D.flat_scene(oracle)
    key = D.morton_keys(g)
    assert np.ptp(g["mu"][:, 1]) == 0 and np.ptp(g["mu"][:, 0]) > 0 and np.ptp(g["mu"][:, 2]) > 0
    assert (key & 0x12492492).max() == 0 and (key & 0x09249249).max() > 0 and (key & 0x24924924).max() > 0   # y bits 0, x and z used


def test_nonfinite_scene_opens_two_leaves_and_leaves_one_clean(oracle):
    g = D.nonfinite_scene(oracle)
    mu = g["mu"][:, :3]
    bad = ~np.isfinite(mu).all(1)
    assert bad.sum() == D.NONFINITE and np.isnan(mu).any() and np.isposinf(mu).any() and np.isneginf(mu).any()
    assert (D.morton_keys(g)[bad] == 0).all()
    leaves = -(-len(g) // D.LEAF)
    opened = D.open_leaves(g)
    assert len(opened) >= 2 and len(opened) < leaves, opened
    assert list(opened[:2]) == [0, 1]                                       # key 0 sorts first: more of them than a leaf holds
    perm = D.morton_order(g)
    assert bad[perm[:D.NONFINITE]].sum() >= D.NONFINITE - 2                 # (a finite centre in the box's corner has key 0 as well)


def test_index_scenes_cover_the_sizes(oracle):
    sc = D.index_scenes(oracle)
    assert set(sc) == set(D.INDEX_NAMES)
    assert [len(sc[f"cloud-{n}"]) for n in (0, 1, 64, 65)] == [0, 1, 64, 65]
    n = len(sc["cloud-4097"])
    leaves = -(-n // D.LEAF)
    assert n == 4097 and leaves == 65 and -(-leaves // D.GROUP) == 2
    for name, g in sc.items():
        assert sorted(D.morton_order(g)) == list(range(len(g))), name
    assert all(len(D.cloud(oracle, n)) == n for n in D.SIZES)


def test_albedo_rule_mirror(oracle):
    for kind in ("albedo4", "albedo-inf"):
        g = B.scene(oracle, ("factors", kind)).g
        assert D.albedo_scale_bits(g["albedo"]) == 4.0 == B.albedo_scale(g), kind
    assert np.isinf(B.scene(oracle, ("factors", "albedo-inf")).g["albedo"]).any()
    assert D.albedo_scale_bits(B.scene(oracle, ("factors", "plain")).g["albedo"]) == 1.0
    g = D.nan_is_the_only_large_albedo(oracle)
    assert np.isnan(g["albedo"]).sum() == 1 and D.albedo_scale_bits(g["albedo"]) == 1.0
    assert D.albedo_scale_bits(D.all_nan_albedo(oracle).g["albedo"]) == 1.0
    assert D.albedo_scale_bits(np.array([[-7.5, 0.5, 0.0, -np.inf]], np.float32)) == 7.5      # the sign does not count
    assert D.albedo_scale_bits(np.zeros((0, 4), np.float32)) == 1.0
    for kind in ("albedo4", "albedo-inf"):
        d = D.dimmed(B.scene(oracle, ("factors", kind)))
        assert D.albedo_scale_bits(d.g["albedo"]) == 1.0 and len(d.g) == len(B.scene(oracle, ("factors", kind)).g)
        assert (d.g["sigma"] == B.scene(oracle, ("factors", kind)).g["sigma"]).all()
