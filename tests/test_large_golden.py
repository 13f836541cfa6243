"""tests/golden/golden_large.json (make_golden_large.py, from the genuine reference): scenes whose scene image does not fit a
workgroup's LDS.  The CPU restatement reproduces the reference's hashes; the GPU side is tests/test_large_scenes.py."""
import os
import sys

import pytest

import support as T

sys.path.insert(0, T.GOLDEN)
import make_golden_large as G  # noqa: E402

CASES = G.load_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_reproduces_the_reference_hashes_of_scenes_too_large_for_lds(name):
    case = CASES[name]
    px, st = T.oracle_render(G.case_scene(case), case["width"], case["height"], case["bounce_limit"], case["rays_per_pixel"],
                             threads=os.cpu_count() or 1)
    assert T.fnv(px) == case["fb_fnv"]
    assert T.fnv(T.oracle_rgb8(px)) == case["rgb8_fnv"]
    assert (st.path_rays, st.shadow_rays) == (case["path_rays"], case["shadow_rays"])


def test_the_goldens_cover_the_regimes_the_issue_names():
    by = {(c["spheres"], c["dir_lights"]) for c in CASES.values()}
    assert any(n >= 2048 for n, _ in by) and (4096, 0) in by and (512, 24) in by
