"""A Pipeline's voxel map to a file and back: save_map writes what Pipeline.mapState() hands out — what the map was made from and
every column it has — into one .npz, load_map merges such a file into a Pipeline's map through Pipeline.mapMergeRows (one fold:
include/madicp_hip.h, madicp_map_merge_rows).  Loading into an empty map restores it — keys, rows, attribute words, evidence
and the ten moment words bit for bit — on either front-end, whichever one saved it; loading into a map that already holds rows
merges the two (evidence adds and saturates, moments add under the freeze rule).  numpy only, nothing is pickled."""
import numpy as np

FORMAT = 1
_COLUMNS = ("attribute", "evidence_words", "moment_words")


def save_map(pipe, path):
    """Writes the map of `pipe` to `path` (numpy appends .npz where the name has no such ending).  Returns the rows written."""
    st = pipe.mapState()
    ev = st["evidence"]
    out = dict(format=np.int64(FORMAT), voxel=np.float64(st["voxel"]), with_attribute=np.bool_(st["with_attribute"]),
               evidence=np.array(ev if ev is not None else (0, 0, 0), np.uint32), moments=np.uint64(st["moments"] or 0),
               keys=np.ascontiguousarray(st["keys"], np.uint64), rows=np.ascontiguousarray(st["rows"], np.float32))
    for name in _COLUMNS:
        if st[name] is not None:
            out[name] = st[name]
    np.savez(path, **out)
    return int(out["keys"].shape[0])


def _spec(voxel, with_attribute, evidence, moments):
    return dict(voxel=float(voxel), with_attribute=bool(with_attribute), evidence=None if evidence is None else tuple(int(v) for v in evidence),
                moments=None if not moments else int(moments))


def load_map(pipe, path):
    """Merges the map saved at `path` into the map of `pipe` — made now, where the pipeline has folded no frame yet.  The file's voxel
    size and column set must be the pipeline's (setMapAccumulation): ValueError names the first difference.  Evidence parameters
    and max_count may differ; they are the pipeline's that apply.  Returns (rows added, rows the map holds)."""
    with np.load(path, allow_pickle=False) as f:
        if int(f["format"]) != FORMAT:
            raise ValueError("load_map: %s has format %d, this reader knows %d" % (path, int(f["format"]), FORMAT))
        ev = tuple(int(v) for v in f["evidence"])
        saved = _spec(f["voxel"], f["with_attribute"], ev if any(ev) else None, int(f["moments"]))
        cols = {name: (f[name] if name in f.files else None) for name in ("keys", "rows") + _COLUMNS}
    if not pipe.mapVoxelSize() > 0:
        raise ValueError("load_map: the pipeline accumulates no map (setMapAccumulation(voxel_size > 0) first)")
    # (asked of the pipeline's options, not of mapState(): that would download every column to read four values)
    if saved["voxel"] != float(pipe.mapVoxelSize()):
        raise ValueError("load_map: the file's voxel size is %r, the pipeline's map has %r" % (saved["voxel"], float(pipe.mapVoxelSize())))
    for in_file, in_map, label in ((saved["with_attribute"], pipe.mapWithAttribute(), "the attribute column"),
                                   (saved["evidence"] is not None, pipe.mapWithEvidence(), "the evidence column"),
                                   (saved["moments"] is not None, pipe.mapWithMoments(), "the moments")):
        if bool(in_file) != bool(in_map):
            which = ("the file has %s and the pipeline's map does not" if in_file else "the pipeline's map has %s and the file does not") % label
            raise ValueError("load_map: " + which)
    return tuple(int(v) for v in pipe.mapMergeRows(cols["keys"], cols["rows"], cols["attribute"], cols["evidence_words"], cols["moment_words"]))
