"""Every map option at once across a front-end switch — attribute, evidence, moments, clearing, the removal log and the overlap query —
on the 8-frame 16 x 450 drive of tests/test_gpu_pipeline_registered_scan.py, deskew off so the folded cloud is the ingested input.
After every frame the frame is restated on a host map of the same spec through capi.host_map_* at the Pipeline's own pose — query,
fold with the attribute, clearing with the previous cursor as watermark — and every column, the new rows, the removed rows and the
frame's overlap counts are held to it byte for byte.  The map lives where frame 0 put it; from frame 3 on the scans come from the
other side and cross over once per frame, their column with them."""
import numpy as np
import pytest

from mad_icp_amd import capi
from test_gpu_pipeline_attribute import with_index
from test_gpu_pipeline_registered_scan import HI, LO, drive, pipeline  # noqa: F401  (drive: the module-scoped fixture)

pytestmark = pytest.mark.gpu

# chosen against the host twin alone, at the drive's ground-truth poses: at 0.5 m with evidence (1, 1, 3) every frame from 1 on
# removes some hundred rows (395 .. 520) and finds 5 600 .. 6 800 of its 6 200 .. 7 200 candidates in the map
VOXEL = 0.5
EVIDENCE = (1, 1, 3)
MOMENTS = 8


@pytest.mark.parametrize("first_frontend", [True, False])
def test_every_option_across_a_front_end_switch(natives, drive, first_frontend):
    p = pipeline(False, first_frontend)
    p.setMapAccumulation(VOXEL, with_attribute=True, evidence=EVIDENCE, moments=MOMENTS)
    p.setMapClearing(True, 0.0)
    p.setMapTrackRemoved(True)
    p.setMapOverlap(True)
    h = capi.host_map_create_mom(VOXEL, 1 << 18, 1 << 24, MOMENTS, with_attr=True, evidence=EVIDENCE)
    try:
        capi.host_map_track_removed(h, True)
        cursor, removed_rows, overlaps = 0, [], []
        for i, f in enumerate(drive):
            if i == 3:
                p.setDeviceFrontEnd(not first_frontend)
            rec, kept, _, _ = with_index(f)
            p.computeRecordsStamped(0.1 * i, rec, LO, HI, attribute="idx")
            T = np.asarray(p.currentPose())
            R, t = T[:3, :3], T[:3, 3]
            # the frame, restated: what the map knew of the scan, the fold, what the scan sees through
            want_overlap = capi.host_map_query(h, f["pts"], R, t, reach=1, per_point=False)
            capi.host_map_insert_attr(h, f["pts"], kept, R, t)
            removed, _, cursor = capi.host_map_clear_rays(h, f["pts"], R, t, margin=0.0, watermark=cursor)
            assert tuple(p.mapFrameOverlap()) == want_overlap, i
            overlaps.append(want_overlap)
            # the consumer's poll: first what left, then what is new
            keys, rows, words = p.mapRemovedRows(with_attribute=True)
            want_keys, want_rows, want_words = capi.host_map_take_removed(h, with_attr=True)
            assert keys.tobytes() == want_keys.tobytes() and rows.tobytes() == want_rows.tobytes(), i
            assert np.asarray(words).tobytes() == want_words.tobytes(), i
            removed_rows.append(want_keys.shape[0])
            rows, words, keys = p.mapNewRows(with_attribute=True, with_keys=True)
            want_rows, want_keys, want_words = capi.host_map_download_rows(h, cursor, with_keys=True, with_attr=True)
            assert rows.tobytes() == want_rows.tobytes() and keys.tobytes() == want_keys.tobytes(), i
            assert np.asarray(words).tobytes() == want_words.tobytes(), i
            cursor = capi.host_map_size(h)
            assert p.mapSize() == cursor and p.mapNewRows().shape[0] == 0
            # every column of the whole map
            rows, words = p.mapCloud(0, with_attribute=True)
            assert rows.tobytes() == capi.host_map_download_f32(h).tobytes(), i
            assert np.asarray(words).tobytes() == capi.host_map_download_attr(h).tobytes(), i
            assert p.mapKeys().tobytes() == capi.host_map_download_keys(h).tobytes(), i
            assert p.mapEvidence().tobytes() == capi.host_map_download_evidence(h).tobytes(), i
            assert p.mapMoments().tobytes() == capi.host_map_download_moments(h).tobytes(), i
        # not vacuous: the log carried rows across the switch, every frame but the first met the map, some row froze its moments
        assert cursor > 1000 and not p.mapOverflowed() and not p.mapRemovedLogFull()
        assert max(removed_rows[:3]) > 0 and max(removed_rows[3:]) > 0, removed_rows
        assert overlaps[0][1] == 0 and all(c[1] > 0 and c[2] > 0 for c in overlaps[1:]), overlaps
        assert int(capi.host_map_download_moments(h)[:, 0].max()) > MOMENTS
    finally:
        capi.host_map_destroy(h)
