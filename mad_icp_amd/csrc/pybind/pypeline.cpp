// pypeline — `Pipeline` + `VectorEigen3d` (reference: mad_icp/src/pybind/pypeline.cpp:57-74).
#include "common.h"
#include "pipeline.h"

#include <algorithm>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

// Pipeline::mapRegister behind mapRegister / mapLinearize: -> (pose (4, 4), info) — info holds H (6, 6), b (6,), chi2 and counts
// (candidates, matched, within, inliers) of the CLOSING linearisation (the one at the returned pose); with `trace` the per-round
// arrays X (K + 1, 12), H_rounds (K + 1, 6, 6), b_rounds (K + 1, 6), chi2_rounds (K + 1,), counts_rounds (K + 1, 4); with `rows`
// (iterations == 0 only) row (n,) int32 and e (n,) float64
static py::tuple map_register_py(Pipeline& self, const py::array_t<double, py::array::c_style | py::array::forcecast>& cloud,
                                 const py::array_t<double, py::array::c_style | py::array::forcecast>& pose, int iterations,
                                 const madicp_host::AlignParams& params, bool trace, bool rows) {
  if (cloud.ndim() != 2 || cloud.shape(1) != 3) throw py::value_error("cloud must be (n, 3)");
  if (pose.ndim() != 2 || pose.shape(0) != 4 || pose.shape(1) != 4) throw py::value_error("pose must be (4, 4)");
  if (iterations < 0 || iterations > madicp_host::kAlignMaxIterations) throw py::value_error("iterations must be 0 .. 64");
  const double* T = pose.data();
  const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
  const double t[3] = {T[3], T[7], T[11]};
  const py::ssize_t n = cloud.shape(0), k1 = iterations + 1;
  std::vector<double> tr(static_cast<size_t>(madicp_host::kAlignTraceRow * k1));
  py::array_t<uint64_t> counts({k1, static_cast<py::ssize_t>(madicp_host::kAlignCounts)});
  py::array_t<int32_t> row(rows ? n : 0);
  py::array_t<double> e(rows ? n : 0);
  double oR[9], ot[3];
  self.mapRegister(cloud.data(), static_cast<size_t>(n), R, t, params, iterations, oR, ot, tr.data(), counts.mutable_data(),
                   rows ? row.mutable_data() : nullptr, rows ? e.mutable_data() : nullptr);
  py::array_t<double> out_pose({4, 4}), X({k1, static_cast<py::ssize_t>(12)}), H({k1, static_cast<py::ssize_t>(6), static_cast<py::ssize_t>(6)}),
      b({k1, static_cast<py::ssize_t>(6)}), chi2(k1);
  double* P = out_pose.mutable_data();
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) P[4 * r + c] = oR[3 * r + c];
    P[4 * r + 3] = ot[r];
  }
  P[12] = P[13] = P[14] = 0.0;
  P[15] = 1.0;
  for (py::ssize_t k = 0; k < k1; ++k) {
    const double* q = tr.data() + madicp_host::kAlignTraceRow * k;
    std::copy(q, q + 12, X.mutable_data() + 12 * k);
    double* Hk = H.mutable_data() + 36 * k;
    int v = 12;
    for (int c = 0; c < 6; ++c)
      for (int r = c; r < 6; ++r) Hk[6 * r + c] = Hk[6 * c + r] = q[v++];
    std::copy(q + 33, q + 39, b.mutable_data() + 6 * k);
    chi2.mutable_data()[k] = q[39];
  }
  py::dict info;
  const py::object last = py::int_(k1 - 1);
  info["H"] = H.attr("__getitem__")(last).attr("copy")();
  info["b"] = b.attr("__getitem__")(last).attr("copy")();
  info["chi2"] = chi2.attr("__getitem__")(last);
  info["counts"] = counts.attr("__getitem__")(last).attr("copy")();
  if (trace) {
    info["X"] = X;
    info["H_rounds"] = H;
    info["b_rounds"] = b;
    info["chi2_rounds"] = chi2;
    info["counts_rounds"] = counts;
  }
  if (rows) {
    info["row"] = row;
    info["e"] = e;
  }
  return py::make_tuple(out_pose, info);
}

// K poses given as (K, 4, 4) or (K, 12) -> the (K, 12) rows Pipeline::mapScorePoses takes: R row-major, then t
static std::vector<double> pose_rows_py(const py::array_t<double, py::array::c_style | py::array::forcecast>& poses) {
  const bool square = poses.ndim() == 3 && poses.shape(1) == 4 && poses.shape(2) == 4;
  if (!square && !(poses.ndim() == 2 && poses.shape(1) == 12)) throw py::value_error("poses must be (K, 4, 4) or (K, 12)");
  const size_t K = static_cast<size_t>(poses.shape(0));
  std::vector<double> rows(12 * std::max<size_t>(K, 1));
  const double* T = poses.data();
  for (size_t k = 0; k < K; ++k) {
    double* X = rows.data() + 12 * k;
    if (!square) {
      std::copy(T + 12 * k, T + 12 * k + 12, X);
      continue;
    }
    for (int r = 0; r < 3; ++r) {
      for (int c = 0; c < 3; ++c) X[3 * r + c] = T[16 * k + 4 * r + c];
      X[9 + r] = T[16 * k + 4 * r + 3];
    }
  }
  return rows;
}

PYBIND11_MODULE(pypeline, m) {
  m.doc() = "mad_icp_amd: MAD-ICP odometry pipeline with the registration on MI355X, drop-in for mad_icp.src.pybind.pypeline";
  // the reference registers the same container in pyvector and pypeline; module_local lets both be imported
  bind_vector_eigen3d(m, py::module_local());
  py::class_<Pipeline>(m, "Pipeline")
    .def(py::init<double, bool, double, double, double, double, double, int, int, bool>(), py::arg("sensor_hz"),
         py::arg("deskew"), py::arg("b_max"), py::arg("rho_ker"), py::arg("p_th"), py::arg("b_min"), py::arg("b_ratio"),
         py::arg("num_keyframes"), py::arg("num_threads"), py::arg("realtime"))
    .def("currentPose", &Pipeline::currentPose)
    .def("trajectory", &Pipeline::trajectory)
    .def("keyframePose", &Pipeline::keyframePose)
    .def("isInitialized", &Pipeline::isInitialized)
    .def("isMapUpdated", &Pipeline::isMapUpdated)
    .def("currentID", &Pipeline::currentID)
    .def("keyframeID", &Pipeline::keyframeID)
    .def("modelLeaves", &Pipeline::modelLeaves)
    .def("currentLeaves", &Pipeline::currentLeaves)
    // compute(stamp, VectorEigen3d): the reference binds the by-value member (pypeline.cpp:69), which has pybind copy the whole
    // container per call; bound here on a reference and handed on as a view — the same call for Python, no 3 MB allocation +
    // copy in front of every frame (the host path makes the one copy its tree keeps, inside)
    .def("compute", [](Pipeline& self, double stamp, const ContainerType& cloud) { self.computeView(stamp, cloud.data(), cloud.size()); })
    // additive: an (N,3) float64 array directly (C-contiguous float64 input is read in place)
    .def("compute",
         [](Pipeline& self, double stamp, py::array_t<double, py::array::c_style | py::array::forcecast> cloud) {
           const Vector3d* pts = points_of_array(cloud);
           self.computeView(stamp, pts, static_cast<size_t>(cloud.shape(0)));
         })
    // additive: compute(stamp, cloud, timestamps) — the acquisition time of every point, normalised to [0, 1] over the scan
    // (what a PointCloud2 reader returns beside the points): with deskew = True the scan is motion-compensated from them
    // instead of the azimuth guess (Pipeline::computeStamped); otherwise exactly compute(stamp, cloud).  A 1-D float64 array
    // (forcecast) of one value per point, ValueError otherwise; the points are read as a view.
    .def("compute",
         [](Pipeline& self, double stamp, const ContainerType& cloud, py::array_t<double, py::array::c_style | py::array::forcecast> ts) {
           if (ts.ndim() != 1 || static_cast<size_t>(ts.shape(0)) != cloud.size())
             throw py::value_error("timestamps must be a 1-D array with one value per point");
           self.computeStampedView(stamp, cloud.data(), ts.data(), cloud.size());
         },
         py::arg("stamp"), py::arg("cloud"), py::arg("timestamps"))
    .def("compute",
         [](Pipeline& self, double stamp, py::array_t<double, py::array::c_style | py::array::forcecast> cloud,
            py::array_t<double, py::array::c_style | py::array::forcecast> ts) {
           const Vector3d* pts = points_of_array(cloud);
           if (ts.ndim() != 1 || ts.shape(0) != cloud.shape(0))
             throw py::value_error("timestamps must be a 1-D array with one value per point");
           self.computeStampedView(stamp, pts, ts.data(), static_cast<size_t>(cloud.shape(0)));
         },
         py::arg("stamp"), py::arg("cloud"), py::arg("timestamps"))
    // additive look-ahead: start building the next scan's MAD-tree while this frame is registered
    .def("lookAheadHits", &Pipeline::lookAheadHits)
    .def("prefetch", [](Pipeline& self, const ContainerType& cloud) { self.prefetchView(cloud.data(), cloud.size()); },
         py::arg("next_cloud"))
    .def("prefetch",
         [](Pipeline& self, py::array_t<double, py::array::c_style | py::array::forcecast> cloud) {
           const Vector3d* pts = points_of_array(cloud);
           self.prefetchView(pts, static_cast<size_t>(cloud.shape(0)));
         })
    // additive: deskew + MAD-tree construction on the device — the default; MAD_ICP_GPU_BUILD=0 or
    // setDeviceFrontEnd(False) keep the host builder
    .def("setDeviceFrontEnd", &Pipeline::setDeviceFrontEnd, py::arg("on"))
    .def("deviceFrontEnd", &Pipeline::deviceFrontEnd)
    // additive: the registered scan out (Pipeline::setKeepScan / registeredScan).  setKeepScan(True) retains the cloud every frame's
    // tree was built from — deskewed where deskew is due — until the next compute*(); registeredScan(voxel_size, frame) returns it
    // as an (M, 3) float32 array in the map frame (frame="map": through currentPose()) or the sensor frame (frame="sensor"), every
    // point (voxel_size = 0) or the lowest-index point of every voxel.  ValueError for another frame name, a voxel_size that is
    // negative or not finite; RuntimeError (std::logic_error) when the option is off or no frame has been computed.
    .def("setKeepScan", &Pipeline::setKeepScan, py::arg("on"))
    .def("keepScan", &Pipeline::keepScan)
    .def("registeredScanSize", &Pipeline::registeredScanSize)
    // ... with_attribute=True: (rows, attr) — attr[j] the attribute of row j, the words the frame carried (computeRecordsStamped's /
    // Source's `attribute`) viewed back as the field's dtype.  RuntimeError (std::logic_error) when the retained scan carries none.
    .def("registeredScan",
         [](Pipeline& self, double voxel_size, const std::string& frame, bool with_attribute) -> py::object {
           if (frame != "map" && frame != "sensor") throw py::value_error("frame must be \"map\" or \"sensor\"");
           const size_t cap = self.registeredScanSize();
           std::vector<float> rows(3 * std::max<size_t>(cap, 1));
           std::vector<uint32_t> words(std::max<size_t>(cap, 1));
           const size_t m = with_attribute ? self.registeredScanWithAttribute(rows.data(), words.data(), cap, voxel_size, frame == "map")
                                           : self.registeredScan(rows.data(), cap, voxel_size, frame == "map");
           py::array_t<float> out({static_cast<py::ssize_t>(m), static_cast<py::ssize_t>(3)});
           if (m) std::memcpy(out.mutable_data(), rows.data(), sizeof(float) * 3 * m);
           if (!with_attribute) return std::move(out);
           py::array_t<uint32_t> w(static_cast<py::ssize_t>(m));
           if (m) std::memcpy(w.mutable_data(), words.data(), sizeof(uint32_t) * m);
           const py::module_ rec = py::module_::import("mad_icp_amd.records");
           return py::make_tuple(out, rec.attr("attribute_view")(w, rec.attr("ATTR_DTYPE")[py::int_(self.registeredScanAttributeType())]));
         },
         py::arg("voxel_size") = 0.0, py::arg("frame") = "map", py::arg("with_attribute") = false)
    // additive: map accumulation (Pipeline::setMapAccumulation).  setMapAccumulation(voxel_size) makes every compute*() end by folding
    // the frame's scan at the frame's pose into an append-only voxel map — the first point ever to fall into a voxel stays — on the
    // device (device front-end) or in its bit-equal host twin; voxel_size = 0 turns it off and frees the map.  mapCloud(first_row)
    // returns rows [first_row, mapSize()) as an (M - first_row, 3) float32 array: what was added since the caller last looked.
    // ValueError for a voxel_size that is negative or not finite, a max_points outside 1 .. 2^30, a first_row beyond the map;
    // RuntimeError (std::logic_error) from mapSize / mapCloud / clearMap while the option is off.
    // with_attribute: the map keeps every row's attribute too; mapCloud(first_row, with_attribute=True) returns (rows, attr), attr
    // viewed as the dtype of the last attribute frame folded (uint32 words before there is one; frames without an attribute
    // contribute zeros).
    // evidence=(hit, miss, cap): the map keeps a hit/miss count per voxel (include/madicp_hip.h has the rule) — folds reinforce,
    // clearings weaken, a row leaves only when its evidence is used up; None (the default) changes nothing.  mapEvidence(first_row=0)
    // returns the words of rows [first_row, mapSize()) as (M,) uint32; mapConfirmed(min_evidence, with_keys=False,
    // with_attribute=False) the rows with evidence >= min_evidence, in row order, compacted where the map lives: (n, 3) float32, or
    // a tuple (rows[, keys][, attr]).  ValueError for hit < 1, miss < 1, cap < hit, cap > 2^31 - 1; RuntimeError (std::logic_error)
    // from both without the column.
    .def("setMapAccumulation",
         [](Pipeline& self, double voxel_size, bool keyframes_only, size_t max_points, bool with_attribute, py::object evidence,
            py::object moments) {
           uint32_t max_count = 0;
           if (!moments.is_none()) {
             const long long v = moments.cast<long long>();
             if (v < 1 || v > 0x80000000ll) throw py::value_error("moments must be None or max_count, 1 .. 2^31");
             max_count = static_cast<uint32_t>(v);
           }
           if (evidence.is_none()) {
             self.setMapAccumulation(voxel_size, keyframes_only, max_points, with_attribute, nullptr, max_count);
             return;
           }
           const py::sequence ev = evidence.cast<py::sequence>();
           if (ev.size() != 3) throw py::value_error("evidence must be None or (hit, miss, cap)");
           uint32_t e[3];
           for (int i = 0; i < 3; ++i) {
             const long long v = ev[i].cast<long long>();
             if (v < 0 || v > 0xffffffffll) throw py::value_error("evidence: hit, miss and cap are 32-bit unsigned values");
             e[i] = static_cast<uint32_t>(v);
           }
           self.setMapAccumulation(voxel_size, keyframes_only, max_points, with_attribute, e, max_count);
         },
         py::arg("voxel_size"), py::arg("keyframes_only") = false, py::arg("max_points") = Pipeline::kMapMaxPointsDefault,
         py::arg("with_attribute") = false, py::arg("evidence") = py::none(), py::arg("moments") = py::none())
    // moments=max_count (1 .. 2^31): the map keeps count, sums and sums of products of the points of every voxel (include/madicp_hip.h
    // has the rule); None (the default) changes nothing.  mapMoments(first_row=0) returns the ten words of rows [first_row, mapSize())
    // as (M, 10) uint64; mapSurfels(first_row=0) returns (centroid (M, 3) float32, normal (M, 3) float32, eigenvalues (M, 3) float32,
    // count (M,) uint32), computed where the map lives.  ValueError outside 1 .. 2^31; RuntimeError (std::logic_error) from both
    // without the moments.
    .def("mapWithMoments", &Pipeline::mapWithMoments)
    .def("mapMoments",
         [](Pipeline& self, size_t first_row) {
           if (!self.mapWithMoments())
             throw std::logic_error("Pipeline::mapMoments: the map was made without moments (setMapAccumulation's moments)");
           const size_t size = self.mapSize();
           if (first_row > size) throw py::value_error("first_row is beyond the map's rows");
           const size_t m = size - first_row;
           py::array_t<uint64_t> w({static_cast<py::ssize_t>(m), static_cast<py::ssize_t>(10)});
           uint64_t no_row[10];
           if (self.mapMoments(m ? w.mutable_data() : no_row, m, first_row) != m)
             throw std::runtime_error("Pipeline::mapMoments: the map changed during the call");
           return w;
         },
         py::arg("first_row") = 0)
    .def("mapSurfels",
         [](Pipeline& self, size_t first_row) {
           if (!self.mapWithMoments())
             throw std::logic_error("Pipeline::mapSurfels: the map was made without moments (setMapAccumulation's moments)");
           const size_t size = self.mapSize();
           if (first_row > size) throw py::value_error("first_row is beyond the map's rows");
           const size_t m = size - first_row;
           const py::ssize_t rows = static_cast<py::ssize_t>(m), three = 3;
           py::array_t<float> c({rows, three}), nrm({rows, three}), eig({rows, three});
           py::array_t<uint32_t> cnt(rows);
           float no_row[3];
           uint32_t no_count[1];
           if (self.mapSurfels(m ? c.mutable_data() : no_row, m ? nrm.mutable_data() : no_row, m ? eig.mutable_data() : no_row,
                               m ? cnt.mutable_data() : no_count, m, first_row) != m)
             throw std::runtime_error("Pipeline::mapSurfels: the map changed during the call");
           return py::make_tuple(c, nrm, eig, cnt);
         },
         py::arg("first_row") = 0)
    .def("mapWithEvidence", &Pipeline::mapWithEvidence)
    .def("mapEvidence",
         [](Pipeline& self, size_t first_row) {
           const size_t size = self.mapSize();
           if (first_row > size) throw py::value_error("first_row is beyond the map's rows");
           const size_t m = size - first_row;
           py::array_t<uint32_t> w(static_cast<py::ssize_t>(m));
           uint32_t no_word[1];
           if (self.mapEvidence(m ? w.mutable_data() : no_word, m, first_row) != m)
             throw std::runtime_error("Pipeline::mapEvidence: the map changed during the call");
           return w;
         },
         py::arg("first_row") = 0)
    .def("mapConfirmed",
         [](Pipeline& self, uint32_t min_evidence, bool with_keys, bool with_attribute) -> py::object {
           if (with_attribute && !self.mapWithAttribute())
             throw std::logic_error("Pipeline::mapConfirmed: the map was made without the attribute (setMapAccumulation's with_attribute)");
           const size_t cap = std::max<size_t>(self.mapSize(), 1);  // (no more rows can qualify than the map holds)
           std::vector<float> xyz(3 * cap);
           std::vector<uint64_t> keys(with_keys ? cap : 0);
           std::vector<uint32_t> words(with_attribute ? cap : 0);
           const size_t n = self.mapConfirmed(min_evidence, xyz.data(), with_keys ? keys.data() : nullptr,
                                              with_attribute ? words.data() : nullptr, nullptr, cap);
           py::array_t<float> out({static_cast<py::ssize_t>(n), static_cast<py::ssize_t>(3)});
           std::copy(xyz.begin(), xyz.begin() + 3 * n, out.mutable_data());
           if (!with_keys && !with_attribute) return std::move(out);
           py::array_t<uint64_t> k(static_cast<py::ssize_t>(with_keys ? n : 0));
           if (with_keys) std::copy(keys.begin(), keys.begin() + n, k.mutable_data());
           py::array_t<uint32_t> w(static_cast<py::ssize_t>(with_attribute ? n : 0));
           if (with_attribute) std::copy(words.begin(), words.begin() + n, w.mutable_data());
           py::object wv = w;
           if (const int type = self.mapAttributeType(); with_attribute && type != madicp_host::kAttrNone) {
             const py::module_ rec = py::module_::import("mad_icp_amd.records");
             wv = rec.attr("attribute_view")(w, rec.attr("ATTR_DTYPE")[py::int_(type)]);
           }
           if (!with_attribute) return py::make_tuple(out, k);
           if (!with_keys) return py::make_tuple(out, wv);
           return py::make_tuple(out, k, wv);
         },
         py::arg("min_evidence"), py::arg("with_keys") = false, py::arg("with_attribute") = false)
    .def("mapWithAttribute", &Pipeline::mapWithAttribute)
    .def("mapVoxelSize", &Pipeline::mapVoxelSize)
    .def("mapOverflowed", &Pipeline::mapOverflowed)
    .def("mapSize", &Pipeline::mapSize)
    .def("mapCloud",
         [](Pipeline& self, size_t first_row, bool with_attribute) -> py::object {
           const size_t size = self.mapSize();
           if (first_row > size) throw py::value_error("first_row is beyond the map's rows");
           const size_t m = size - first_row;
           py::array_t<float> out({static_cast<py::ssize_t>(m), static_cast<py::ssize_t>(3)});
           float none[3];
           if (self.mapCloud(m ? out.mutable_data() : none, m, first_row) != m)
             throw std::runtime_error("Pipeline::mapCloud: the map changed during the call");
           if (!with_attribute) return std::move(out);
           py::array_t<uint32_t> w(static_cast<py::ssize_t>(m));
           uint32_t no_word[1];
           if (self.mapAttribute(m ? w.mutable_data() : no_word, m, first_row) != m)
             throw std::runtime_error("Pipeline::mapCloud: the map changed during the call");
           const int type = self.mapAttributeType();
           if (type == madicp_host::kAttrNone) return py::make_tuple(out, w);
           const py::module_ rec = py::module_::import("mad_icp_amd.records");
           return py::make_tuple(out, rec.attr("attribute_view")(w, rec.attr("ATTR_DTYPE")[py::int_(type)]));
         },
         py::arg("first_row") = 0, py::arg("with_attribute") = false)
    .def("clearMap", &Pipeline::clearMap)
    // additive: a map that follows the vehicle (Pipeline::setMapRange).  setMapRange(radius) lets every fold prune the rows farther
    // than radius from the vehicle once it has moved radius / 4 since the last prune, and before a fold that max_points would
    // refuse; 0 (the default) turns it off.  mapPrune(center, radius) does it by hand and returns the rows removed; mapRemoved()
    // counts them.  mapNewRows(with_attribute=False) returns the rows added since the previous call as (M, 3) float32, or
    // (rows, attr): the incremental consumer's call — across prunes every row is delivered at most once (a row added and pruned
    // between two calls: never).  ValueError for a radius that is negative or not finite or whose square is not finite, a
    // non-finite center; RuntimeError (std::logic_error) from mapPrune / mapNewRows while accumulation is off.
    .def("setMapRange", &Pipeline::setMapRange, py::arg("radius"))
    .def("mapRange", &Pipeline::mapRange)
    .def("mapRemoved", &Pipeline::mapRemoved)
    .def("mapPrune",
         [](Pipeline& self, py::array_t<double, py::array::c_style | py::array::forcecast> center, double radius) {
           if (center.size() != 3) throw py::value_error("center must hold 3 values");
           return self.mapPrune(center.data(), radius);
         },
         py::arg("center"), py::arg("radius"))
    // additive: free-space clearing (Pipeline::setMapClearing).  setMapClearing(on, margin=0, origin=(0, 0, 0)) lets every fold
    // remove the rows whose voxel a ray of the folded scan is sampled in and no point of that scan lies in; off by default.
    // mapClearRays(cloud (n, 3), pose (4, 4), origin=(0, 0, 0), margin=0) does it by hand and returns the rows removed;
    // mapRemoved() counts prunes and clearings together.  ValueError for a margin that is negative or not finite, a non-finite
    // origin or pose; RuntimeError (std::logic_error) from mapClearRays while accumulation is off.
    .def("setMapClearing",
         [](Pipeline& self, bool on, double margin, py::array_t<double, py::array::c_style | py::array::forcecast> origin) {
           if (origin.size() != 3) throw py::value_error("origin must hold 3 values");
           self.setMapClearing(on, margin, origin.data());
         },
         py::arg("on"), py::arg("margin") = 0.0, py::arg("origin") = std::vector<double>{0.0, 0.0, 0.0})
    .def("mapClearing", &Pipeline::mapClearing)
    .def("mapClearRays",
         [](Pipeline& self, py::array_t<double, py::array::c_style | py::array::forcecast> cloud,
            py::array_t<double, py::array::c_style | py::array::forcecast> pose,
            py::array_t<double, py::array::c_style | py::array::forcecast> origin, double margin) {
           if (cloud.ndim() != 2 || cloud.shape(1) != 3) throw py::value_error("cloud must be (n, 3)");
           if (pose.ndim() != 2 || pose.shape(0) != 4 || pose.shape(1) != 4) throw py::value_error("pose must be (4, 4)");
           if (origin.size() != 3) throw py::value_error("origin must hold 3 values");
           const double* T = pose.data();
           const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
           const double t[3] = {T[3], T[7], T[11]};
           return self.mapClearRays(cloud.data(), static_cast<size_t>(cloud.shape(0)), R, t, origin.data(), margin);
         },
         py::arg("cloud"), py::arg("pose"), py::arg("origin") = std::vector<double>{0.0, 0.0, 0.0}, py::arg("margin") = 0.0)
    // additive: asking the map (Pipeline::mapQuery).  mapQuery(cloud (n, 3), pose (4, 4), reach=1, max_dist=inf, with_keys=False,
    // with_attribute=False, with_evidence=False) returns (counts, row (n,) int32, d2 (n,) float64[, keys uint64][, attr][, ev uint32]):
    // per point the nearest map row of its voxel neighbourhood (-1, +inf, all ones, 0 where there is none), counts = (candidates,
    // matched, within max_dist); attr viewed as the field's dtype as in mapCloud.  mapOverlap(cloud, pose, reach=1, max_dist=inf)
    // returns the three counts alone: the scoring form, no per-point copy.  setMapOverlap(on, reach=1, max_dist=inf) makes every fold
    // ask the map about the frame first; mapFrameOverlap() returns that frame's counts (zeros for a frame that was not folded).
    // ValueError for a reach other than 0 and 1, a max_dist that is NaN or negative, a non-finite pose; RuntimeError (std::logic_error)
    // while accumulation is off and for a column the map lacks.
    .def("mapQuery",
         [](Pipeline& self, py::array_t<double, py::array::c_style | py::array::forcecast> cloud,
            py::array_t<double, py::array::c_style | py::array::forcecast> pose, int reach, double max_dist, bool with_keys,
            bool with_attribute, bool with_evidence) -> py::object {
           if (cloud.ndim() != 2 || cloud.shape(1) != 3) throw py::value_error("cloud must be (n, 3)");
           if (pose.ndim() != 2 || pose.shape(0) != 4 || pose.shape(1) != 4) throw py::value_error("pose must be (4, 4)");
           const double* T = pose.data();
           const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
           const double t[3] = {T[3], T[7], T[11]};
           const py::ssize_t n = cloud.shape(0);
           py::array_t<int32_t> row(n);
           py::array_t<double> d2(n);
           py::array_t<uint64_t> k(with_keys ? n : 0);
           py::array_t<uint32_t> w(with_attribute ? n : 0), e(with_evidence ? n : 0);
           uint64_t counts[3] = {0, 0, 0};
           self.mapQuery(cloud.data(), static_cast<size_t>(n), R, t, reach, max_dist, row.mutable_data(), d2.mutable_data(),
                         with_keys ? k.mutable_data() : nullptr, with_attribute ? w.mutable_data() : nullptr,
                         with_evidence ? e.mutable_data() : nullptr, counts);
           py::list out;
           out.append(py::make_tuple(counts[0], counts[1], counts[2]));
           out.append(row);
           out.append(d2);
           if (with_keys) out.append(k);
           if (with_attribute) {
             py::object words = w;
             if (const int type = self.mapAttributeType(); type != madicp_host::kAttrNone) {
               const py::module_ rec = py::module_::import("mad_icp_amd.records");
               words = rec.attr("attribute_view")(w, rec.attr("ATTR_DTYPE")[py::int_(type)]);
             }
             out.append(words);
           }
           if (with_evidence) out.append(e);
           return py::tuple(out);
         },
         py::arg("cloud"), py::arg("pose"), py::arg("reach") = 1, py::arg("max_dist") = madicp_host::kQueryNoDistance,
         py::arg("with_keys") = false, py::arg("with_attribute") = false, py::arg("with_evidence") = false)
    .def("mapOverlap",
         [](Pipeline& self, py::array_t<double, py::array::c_style | py::array::forcecast> cloud,
            py::array_t<double, py::array::c_style | py::array::forcecast> pose, int reach, double max_dist) {
           if (cloud.ndim() != 2 || cloud.shape(1) != 3) throw py::value_error("cloud must be (n, 3)");
           if (pose.ndim() != 2 || pose.shape(0) != 4 || pose.shape(1) != 4) throw py::value_error("pose must be (4, 4)");
           const double* T = pose.data();
           const double R[9] = {T[0], T[1], T[2], T[4], T[5], T[6], T[8], T[9], T[10]};
           const double t[3] = {T[3], T[7], T[11]};
           uint64_t counts[3] = {0, 0, 0};
           self.mapQuery(cloud.data(), static_cast<size_t>(cloud.shape(0)), R, t, reach, max_dist, nullptr, nullptr, nullptr, nullptr, nullptr,
                         counts);
           return py::make_tuple(counts[0], counts[1], counts[2]);
         },
         py::arg("cloud"), py::arg("pose"), py::arg("reach") = 1, py::arg("max_dist") = madicp_host::kQueryNoDistance)
    .def("setMapOverlap", &Pipeline::setMapOverlap, py::arg("on"), py::arg("reach") = 1, py::arg("max_dist") = madicp_host::kQueryNoDistance)
    .def("mapFrameOverlap",
         [](const Pipeline& self) {
           const uint64_t* c = self.mapFrameOverlap();
           return py::make_tuple(c[0], c[1], c[2]);
         })
    // additive: registering a scan against the map's surfels (Pipeline::mapRegister).  mapRegister(cloud (n, 3), pose (4, 4),
    // iterations, reach=1, max_dist=inf, rho=inf, min_count=3, flat=1.0, trace=False) returns (pose (4, 4), info): the pose after
    // `iterations` Gauss-Newton rounds, and H (6, 6), b, chi2, counts of the linearisation AT that pose (plus the per-round arrays
    // with trace).  The defaults are the neutral parameters, not tuned ones.  mapLinearize(cloud, pose, ..., with_rows=False) is the
    // iterations = 0 form: the pose comes back as given, with_rows adds the per-point row and e.  ValueError for what
    // madicp_map_register_cloud refuses; RuntimeError (std::logic_error) while accumulation is off or without moments.
    .def("mapRegister",
         [](Pipeline& self, py::array_t<double, py::array::c_style | py::array::forcecast> cloud,
            py::array_t<double, py::array::c_style | py::array::forcecast> pose, int iterations, int reach, double max_dist, double rho,
            uint32_t min_count, double flat, bool trace) {
           return map_register_py(self, cloud, pose, iterations, madicp_host::AlignParams{reach, max_dist, rho, min_count, flat}, trace, false);
         },
         py::arg("cloud"), py::arg("pose"), py::arg("iterations"), py::arg("reach") = 1, py::arg("max_dist") = madicp_host::kQueryNoDistance,
         py::arg("rho") = madicp_host::kQueryNoDistance, py::arg("min_count") = 3, py::arg("flat") = 1.0, py::arg("trace") = false)
    .def("mapLinearize",
         [](Pipeline& self, py::array_t<double, py::array::c_style | py::array::forcecast> cloud,
            py::array_t<double, py::array::c_style | py::array::forcecast> pose, int reach, double max_dist, double rho, uint32_t min_count,
            double flat, bool with_rows) {
           return map_register_py(self, cloud, pose, 0, madicp_host::AlignParams{reach, max_dist, rho, min_count, flat}, false, with_rows);
         },
         py::arg("cloud"), py::arg("pose"), py::arg("reach") = 1, py::arg("max_dist") = madicp_host::kQueryNoDistance,
         py::arg("rho") = madicp_host::kQueryNoDistance, py::arg("min_count") = 3, py::arg("flat") = 1.0, py::arg("with_rows") = false)
    // additive: many hypotheses (Pipeline::mapScorePoses / mapRelocalize).  mapScorePoses(cloud (n, 3), poses (K, 4, 4) or (K, 12),
    // reach=1, max_dist=inf, stride=1) returns (K, 3) uint64: mapOverlap's three counts of cloud[::stride] at every pose, one call
    // and one host synchronisation.  mapRelocalize(cloud, poses, refine=4, iterations=10, stride=8, reach=1, max_dist=inf, rho=inf,
    // min_count=3, flat=1.0) scores all K poses (stride), ranks them by (within descending, index ascending) and registers the first
    // min(refine, K) with every point, as mapRegister does; it returns a dict, one entry per refined hypothesis in rank order: index
    // (m,) int32, scores (m, 3) uint64, poses (m, 4, 4), H (m, 6, 6), b (m, 6), chi2 (m,), counts (m, 4) of the closing
    // linearisation, and best: the entry with the most closing inliers (a tie to the better rank).  reach and max_dist serve both the
    // scoring and the registration.  ValueError for what the calls refuse and for refine outside 1 .. 64; RuntimeError
    // (std::logic_error) while accumulation is off and, for mapRelocalize, without moments.
    .def("mapScorePoses",
         [](Pipeline& self, py::array_t<double, py::array::c_style | py::array::forcecast> cloud,
            py::array_t<double, py::array::c_style | py::array::forcecast> poses, int reach, double max_dist, int64_t stride) {
           if (cloud.ndim() != 2 || cloud.shape(1) != 3) throw py::value_error("cloud must be (n, 3)");
           const std::vector<double> rows = pose_rows_py(poses);
           const py::ssize_t K = poses.shape(0);
           py::array_t<uint64_t> counts({K, static_cast<py::ssize_t>(3)});
           std::vector<uint64_t> got(3 * std::max<size_t>(static_cast<size_t>(K), 1));
           self.mapScorePoses(cloud.data(), static_cast<size_t>(cloud.shape(0)), rows.data(), static_cast<size_t>(K), reach, max_dist, stride,
                              got.data());
           std::copy(got.begin(), got.begin() + 3 * K, counts.mutable_data());
           return counts;
         },
         py::arg("cloud"), py::arg("poses"), py::arg("reach") = 1, py::arg("max_dist") = madicp_host::kQueryNoDistance, py::arg("stride") = 1)
    .def("mapRelocalize",
         [](Pipeline& self, py::array_t<double, py::array::c_style | py::array::forcecast> cloud,
            py::array_t<double, py::array::c_style | py::array::forcecast> poses, int refine, int iterations, int64_t stride, int reach,
            double max_dist, double rho, uint32_t min_count, double flat) {
           if (cloud.ndim() != 2 || cloud.shape(1) != 3) throw py::value_error("cloud must be (n, 3)");
           if (refine < 1 || refine > Pipeline::kRelocalizeMaxRefine) throw py::value_error("refine must be 1 .. 64");
           const std::vector<double> rows = pose_rows_py(poses);
           const size_t K = static_cast<size_t>(poses.shape(0)), cap = static_cast<size_t>(refine);
           std::vector<int32_t> index(cap);
           std::vector<uint64_t> scores(3 * cap), counts(madicp_host::kAlignCounts * cap);
           std::vector<double> X(12 * cap), sums(madicp_host::kAlignTerms * cap);
           size_t best = 0;
           const py::ssize_t m = static_cast<py::ssize_t>(
               self.mapRelocalize(cloud.data(), static_cast<size_t>(cloud.shape(0)), rows.data(), K, reach, max_dist, stride, refine,
                                  madicp_host::AlignParams{reach, max_dist, rho, min_count, flat}, iterations, index.data(), scores.data(),
                                  X.data(), sums.data(), counts.data(), &best));
           py::array_t<int32_t> o_index(m);
           py::array_t<uint64_t> o_scores({m, static_cast<py::ssize_t>(3)}), o_counts({m, static_cast<py::ssize_t>(madicp_host::kAlignCounts)});
           py::array_t<double> o_poses({m, static_cast<py::ssize_t>(4), static_cast<py::ssize_t>(4)}),
               H({m, static_cast<py::ssize_t>(6), static_cast<py::ssize_t>(6)}), b({m, static_cast<py::ssize_t>(6)}), chi2(m);
           std::copy(index.begin(), index.begin() + m, o_index.mutable_data());
           std::copy(scores.begin(), scores.begin() + 3 * m, o_scores.mutable_data());
           std::copy(counts.begin(), counts.begin() + madicp_host::kAlignCounts * m, o_counts.mutable_data());
           for (py::ssize_t r = 0; r < m; ++r) {
             double* P = o_poses.mutable_data() + 16 * r;
             for (int i = 0; i < 3; ++i) {
               for (int c = 0; c < 3; ++c) P[4 * i + c] = X[12 * r + 3 * i + c];
               P[4 * i + 3] = X[12 * r + 9 + i];
             }
             P[12] = P[13] = P[14] = 0.0;
             P[15] = 1.0;
             const double* q = sums.data() + madicp_host::kAlignTerms * r;
             double* Hr = H.mutable_data() + 36 * r;
             int v = 0;
             for (int c = 0; c < 6; ++c)
               for (int i = c; i < 6; ++i) Hr[6 * i + c] = Hr[6 * c + i] = q[v++];
             std::copy(q + 21, q + 27, b.mutable_data() + 6 * r);
             chi2.mutable_data()[r] = q[27];
           }
           py::dict out;
           out["index"] = o_index;
           out["scores"] = o_scores;
           out["poses"] = o_poses;
           out["H"] = H;
           out["b"] = b;
           out["chi2"] = chi2;
           out["counts"] = o_counts;
           out["best"] = py::int_(best);
           return out;
         },
         py::arg("cloud"), py::arg("poses"), py::arg("refine") = 4, py::arg("iterations") = 10, py::arg("stride") = 8, py::arg("reach") = 1,
         py::arg("max_dist") = madicp_host::kQueryNoDistance, py::arg("rho") = madicp_host::kQueryNoDistance, py::arg("min_count") = 3,
         py::arg("flat") = 1.0)
    // additive: saved rows back in (Pipeline::mapMergeRows).  mapState() returns a dict: what the map was made from — voxel,
    // with_attribute, evidence ((hit, miss, cap) or None), moments (max_count or None) — and its columns through the window downloads:
    // keys (M,) uint64, rows (M, 3) float32, attribute (M,) uint32 or None, evidence_words (M,) uint32 or None, moment_words (M, 10)
    // uint64 or None.  mapMergeRows(keys, rows, attribute=None, evidence=None, moments=None) merges such columns into this pipeline's
    // map as ONE fold — before the first frame too: the map is then made — and returns (added, size); a column is given exactly
    // where the map has it.  Attribute words travel as uint32: an array of another 4-byte dtype is taken by its bits, never
    // converted.  mad_icp_amd.map_io has save_map / load_map over the two.  ValueError for what madicp_map_merge_rows refuses as
    // invalid and for columns of unequal length; RuntimeError for a capacity refusal and while accumulation is off.
    .def("mapState",
         [](Pipeline& self) {
           if (self.mapVoxelSize() == 0.0) throw std::logic_error("Pipeline::mapState: setMapAccumulation(voxel_size > 0) first");
           const size_t m = self.mapSize();
           const py::ssize_t rows = static_cast<py::ssize_t>(m);
           py::dict out;
           out["voxel"] = self.mapVoxelSize();
           out["with_attribute"] = self.mapWithAttribute();
           const uint32_t* e = self.mapEvidenceParams();
           out["evidence"] = self.mapWithEvidence() ? py::object(py::make_tuple(e[0], e[1], e[2])) : py::object(py::none());
           out["moments"] = self.mapWithMoments() ? py::object(py::int_(self.mapMomentsMaxCount())) : py::object(py::none());
           auto took = [&](size_t got) {
             if (got != m) throw std::runtime_error("Pipeline::mapState: the map changed during the call");
           };
           py::array_t<uint64_t> keys(rows);
           py::array_t<float> xyz({rows, static_cast<py::ssize_t>(3)});
           uint64_t no_key[10];
           float none[3];
           uint32_t no_word[1];
           took(self.mapKeys(m ? keys.mutable_data() : no_key, m, 0));
           took(self.mapCloud(m ? xyz.mutable_data() : none, m, 0));
           out["keys"] = keys;
           out["rows"] = xyz;
           out["attribute"] = py::none();
           out["evidence_words"] = py::none();
           out["moment_words"] = py::none();
           if (self.mapWithAttribute()) {
             py::array_t<uint32_t> w(rows);
             took(self.mapAttribute(m ? w.mutable_data() : no_word, m, 0));
             out["attribute"] = w;
           }
           if (self.mapWithEvidence()) {
             py::array_t<uint32_t> w(rows);
             took(self.mapEvidence(m ? w.mutable_data() : no_word, m, 0));
             out["evidence_words"] = w;
           }
           if (self.mapWithMoments()) {
             py::array_t<uint64_t> w({rows, static_cast<py::ssize_t>(10)});
             took(self.mapMoments(m ? w.mutable_data() : no_key, m, 0));
             out["moment_words"] = w;
           }
           return out;
         })
    .def("mapMergeRows",
         [](Pipeline& self, py::array_t<uint64_t, py::array::c_style> keys, py::array_t<float, py::array::c_style> rows, py::object attribute,
            py::object evidence_words, py::object moment_words) {
           if (keys.ndim() != 1) throw py::value_error("keys must be (n,) uint64");
           const py::ssize_t n = keys.shape(0);
           if (rows.ndim() != 2 || rows.shape(0) != n || rows.shape(1) != 3) throw py::value_error("rows must be (n, 3) float32");
           py::array_t<uint32_t, py::array::c_style> words;
           const bool with_attr = !attribute.is_none(), with_ev = !evidence_words.is_none(), with_mom = !moment_words.is_none();
           py::array_t<uint32_t, py::array::c_style> evidence;
           py::array_t<uint64_t, py::array::c_style> moments;
           if (with_ev) evidence = evidence_words.cast<py::array_t<uint32_t, py::array::c_style>>();
           if (with_mom) moments = moment_words.cast<py::array_t<uint64_t, py::array::c_style>>();
           if (with_attr) {  // (the bits of a 4-byte dtype, whatever it is: a float32 attribute is not converted to integers)
             py::array a = py::module_::import("numpy").attr("ascontiguousarray")(attribute);
             if (a.itemsize() != 4) throw py::value_error("attribute must have a 4-byte dtype (its words travel as uint32)");
             words = a.attr("view")("uint32");
             if (words.ndim() != 1 || words.shape(0) != n) throw py::value_error("attribute must be (n,)");
           }
           if (with_ev && (evidence.ndim() != 1 || evidence.shape(0) != n)) throw py::value_error("evidence must be (n,) uint32");
           if (with_mom && (moments.ndim() != 2 || moments.shape(0) != n || moments.shape(1) != 10))
             throw py::value_error("moments must be (n, 10) uint64");
           size_t added = 0;
           try {
             const size_t size = self.mapMergeRows(keys.data(), rows.data(), with_attr ? words.data() : nullptr,
                                                   with_ev ? evidence.data() : nullptr, with_mom ? moments.data() : nullptr,
                                                   static_cast<size_t>(n), &added);
             return py::make_tuple(added, size);
           } catch (const std::invalid_argument& e) {
             throw py::value_error(e.what());
           }
         },
         py::arg("keys"), py::arg("rows"), py::arg("attribute") = py::none(), py::arg("evidence") = py::none(),
         py::arg("moments") = py::none())
    // setMapAlignment(on, iterations=5, reach=1, max_dist=inf, rho=inf, min_count=3, flat=1.0) makes every fold register the frame
    // against the map first and only REPORT it; mapFrameAlignment() returns None for a frame without one, else (pose (4, 4), info) with
    // H, b, chi2, counts at that pose and chi2_start, counts_start at the frame's own.
    .def("setMapAlignment",
         [](Pipeline& self, bool on, int iterations, int reach, double max_dist, double rho, uint32_t min_count, double flat) {
           self.setMapAlignment(on, iterations, madicp_host::AlignParams{reach, max_dist, rho, min_count, flat});
         },
         py::arg("on"), py::arg("iterations") = 5, py::arg("reach") = 1, py::arg("max_dist") = madicp_host::kQueryNoDistance,
         py::arg("rho") = madicp_host::kQueryNoDistance, py::arg("min_count") = 3, py::arg("flat") = 1.0)
    .def("mapFrameAlignment",
         [](const Pipeline& self) -> py::object {
           const Pipeline::FrameAlignment& a = self.mapFrameAlignment();
           if (!a.valid) return py::none();
           py::array_t<double> pose({4, 4}), H({6, 6}), b(6);
           py::array_t<uint64_t> counts(madicp_host::kAlignCounts), first(madicp_host::kAlignCounts);
           double* P = pose.mutable_data();
           for (int r = 0; r < 3; ++r) {
             for (int c = 0; c < 3; ++c) P[4 * r + c] = a.R[3 * r + c];
             P[4 * r + 3] = a.t[r];
           }
           P[12] = P[13] = P[14] = 0.0;
           P[15] = 1.0;
           int v = 0;
           for (int c = 0; c < 6; ++c)
             for (int r = c; r < 6; ++r) H.mutable_data()[6 * r + c] = H.mutable_data()[6 * c + r] = a.sums[v++];
           std::copy(a.sums + 21, a.sums + 27, b.mutable_data());
           std::copy(a.counts, a.counts + madicp_host::kAlignCounts, counts.mutable_data());
           std::copy(a.first_counts, a.first_counts + madicp_host::kAlignCounts, first.mutable_data());
           py::dict info;
           info["iterations"] = a.iterations;
           info["H"] = H;
           info["b"] = b;
           info["chi2"] = a.sums[27];
           info["counts"] = counts;
           info["chi2_start"] = a.first_chi2;
           info["counts_start"] = first;
           return py::make_tuple(pose, info);
         })
    .def("mapNewRows",
         [](Pipeline& self, bool with_attribute, bool with_keys) -> py::object {
           const size_t m = self.mapNewRowCount();
           if (with_attribute && !self.mapWithAttribute())
             throw std::logic_error("Pipeline::mapNewRows: the map was made without the attribute (setMapAccumulation's with_attribute)");
           py::array_t<float> out({static_cast<py::ssize_t>(m), static_cast<py::ssize_t>(3)});
           py::array_t<uint32_t> w(static_cast<py::ssize_t>(with_attribute ? m : 0));
           py::array_t<uint64_t> k(static_cast<py::ssize_t>(with_keys ? m : 0));
           float none[3];
           uint32_t no_word[1];
           uint64_t no_key[1];
           if (self.mapNewRows(m ? out.mutable_data() : none, m, with_attribute ? (m ? w.mutable_data() : no_word) : nullptr,
                               with_keys ? (m ? k.mutable_data() : no_key) : nullptr) != m)
             throw std::runtime_error("Pipeline::mapNewRows: the map changed during the call");
           if (!with_attribute && !with_keys) return std::move(out);
           py::object words = w;
           if (const int type = self.mapAttributeType(); with_attribute && type != madicp_host::kAttrNone) {
             const py::module_ rec = py::module_::import("mad_icp_amd.records");
             words = rec.attr("attribute_view")(w, rec.attr("ATTR_DTYPE")[py::int_(type)]);
           }
           if (!with_keys) return py::make_tuple(out, words);
           if (!with_attribute) return py::make_tuple(out, k);
           return py::make_tuple(out, words, k);
         },
         py::arg("with_attribute") = false, py::arg("with_keys") = false)
    // additive: a map that a consumer can mirror (Pipeline::setMapTrackRemoved).  mapKeys(first_row=0): the stored 64-bit voxel keys of
    // rows [first_row, mapSize()), uint64 (M,) — a row's identity across prunes; mapNewRows(with_keys=True) puts the new rows' keys
    // last in the tuple.  setMapTrackRemoved(True) makes the map log the rows that were delivered through mapNewRows and have left
    // since; mapRemovedRows(with_attribute=False) takes the log as (keys uint64 (n,), rows float32 (n, 3)[, attr]), attr viewed as the
    // field's dtype as in mapNewRows.  mapRemovedLogFull(): a removal was skipped because the log held max_points entries — true
    // until the next mapRemovedRows().  mad_icp_amd.map_mirror.MapMirror is the reference consumer.  RuntimeError (std::logic_error)
    // while accumulation is off, from mapRemovedRows while tracking is off.
    .def("setMapTrackRemoved", &Pipeline::setMapTrackRemoved, py::arg("on"))
    .def("mapTrackRemoved", &Pipeline::mapTrackRemoved)
    .def("mapRemovedRowCount", &Pipeline::mapRemovedRowCount)
    .def("mapRemovedLogFull", &Pipeline::mapRemovedLogFull)
    .def("mapRemovedRows",
         [](Pipeline& self, bool with_attribute) -> py::object {
           const size_t m = self.mapRemovedRowCount();
           if (with_attribute && !self.mapWithAttribute())
             throw std::logic_error("Pipeline::mapRemovedRows: the map was made without the attribute (setMapAccumulation's with_attribute)");
           py::array_t<uint64_t> k(static_cast<py::ssize_t>(m));
           py::array_t<float> out({static_cast<py::ssize_t>(m), static_cast<py::ssize_t>(3)});
           py::array_t<uint32_t> w(static_cast<py::ssize_t>(with_attribute ? m : 0));
           uint64_t no_key[1];
           float none[3];
           uint32_t no_word[1];
           if (self.mapRemovedRows(m ? k.mutable_data() : no_key, m ? out.mutable_data() : none,
                                   with_attribute ? (m ? w.mutable_data() : no_word) : nullptr, m) != m)
             throw std::runtime_error("Pipeline::mapRemovedRows: the log changed during the call");
           if (!with_attribute) return py::make_tuple(k, out);
           const int type = self.mapAttributeType();
           if (type == madicp_host::kAttrNone) return py::make_tuple(k, out, w);
           const py::module_ rec = py::module_::import("mad_icp_amd.records");
           return py::make_tuple(k, out, rec.attr("attribute_view")(w, rec.attr("ATTR_DTYPE")[py::int_(type)]));
         },
         py::arg("with_attribute") = false)
    .def("mapKeys",
         [](Pipeline& self, size_t first_row) {
           const size_t size = self.mapSize();
           if (first_row > size) throw py::value_error("first_row is beyond the map's rows");
           const size_t m = size - first_row;
           py::array_t<uint64_t> k(static_cast<py::ssize_t>(m));
           uint64_t no_key[1];
           if (self.mapKeys(m ? k.mutable_data() : no_key, m, first_row) != m)
             throw std::runtime_error("Pipeline::mapKeys: the map changed during the call");
           return k;
         },
         py::arg("first_row") = 0)
    // additive: a frame straight from sensor records, (n, >=3) float32 (a KITTI .bin is (n,4)): range filter, optional
    // KITTI correction (apps/cpp_runners/bin_runner.cpp:126-166), deskew, build and registration on the device
    .def("computeRecords",
         [](Pipeline& self, double stamp, py::array_t<float, py::array::c_style | py::array::forcecast> rec, double min_range,
            double max_range, bool kitti) {
           if (rec.ndim() != 2 || rec.shape(1) < 3) throw py::cast_error("records must be an (n, >=3) float32 array");
           self.computeRecords(stamp, rec.data(), static_cast<size_t>(rec.shape(0)), static_cast<int>(rec.shape(1)), min_range,
                               max_range, kitti);
         },
         py::arg("stamp"), py::arg("records"), py::arg("min_range"), py::arg("max_range"), py::arg("kitti_correction") = false)
    // additive: a frame straight from a driver's byte records WITH a time field (Pipeline::computeRecordsStamped): a C-contiguous
    // 1-D numpy structured array — what a PointCloud2 reader returns — whose layout mad_icp_amd.records reads off the dtype
    // (x, y, z float32; the time field by name, default the first of t / timestamp / time present; time_field=False: none), or
    // an (n, point_step) uint8 array with an explicit layout = (point_step, off_x, off_y, off_z, off_t, t_type).  The array
    // is read in place.  time_range: None = the min / max time over the message, else (t_begin, t_end).  ValueError for what the
    // helper or the ingest refuses.
    .def("computeRecordsStamped",
         [](Pipeline& self, double stamp, py::array rec, double min_range, double max_range, bool kitti, py::object time_field,
            py::object time_range, py::object layout, py::object attribute) {
           const py::tuple r = py::module_::import("mad_icp_amd.records").attr("resolve")(rec, time_field, layout);
           const size_t n = r[0].cast<size_t>();
           const py::tuple l = r[1];
           const madicp_host::RecordLayout L{l[0].cast<int32_t>(), l[1].cast<int32_t>(), l[2].cast<int32_t>(),
                                             l[3].cast<int32_t>(), l[4].cast<int32_t>(), l[5].cast<int32_t>()};
           double range[2];
           const bool have_range = !time_range.is_none();
           if (have_range) {
             const py::sequence tr = time_range.cast<py::sequence>();
             if (py::len(tr) != 2) throw py::value_error("time_range must be (t_begin, t_end)");
             range[0] = tr[0].cast<double>();
             range[1] = tr[1].cast<double>();
           }
           madicp_host::AttrField A{0, madicp_host::kAttrNone};
           if (!attribute.is_none()) {  // (a field's name, or (offset, type code) for raw records: mad_icp_amd.records.resolve_attribute)
             const py::tuple a = py::module_::import("mad_icp_amd.records").attr("resolve_attribute")(rec, attribute);
             A = madicp_host::AttrField{a[0].cast<int32_t>(), a[1].cast<int32_t>()};
           }
           try {
             if (!attribute.is_none())
               self.computeRecordsStamped(stamp, rec.data(), n, L, min_range, max_range, kitti, have_range ? range : nullptr, A);
             else
               self.computeRecordsStamped(stamp, rec.data(), n, L, min_range, max_range, kitti, have_range ? range : nullptr);
           } catch (const std::invalid_argument& e) {
             throw py::value_error(e.what());
           }
         },
         py::arg("stamp"), py::arg("records"), py::arg("min_range"), py::arg("max_range"), py::arg("kitti_correction") = false,
         py::arg("time_field") = py::none(), py::arg("time_range") = py::none(), py::arg("layout") = py::none(),
         py::arg("attribute") = py::none())
    // additive: a frame from SEVERAL sensors' byte records (Pipeline::computeSourcesStamped): a sequence of
    // mad_icp_amd.records.Source — the buffer as computeRecordsStamped takes it, the range bounds in the sensor's frame, the 4x4
    // sensor_to_base and the time field's scale / offset onto the common clock.  The arrays are read in place.  time_range:
    // None = the min / max over all sources on the common clock, else (t_begin, t_end) there.  ValueError for what the helper or
    // the ingest refuses.
    .def("computeSourcesStamped",
         [](Pipeline& self, double stamp, py::object sources, py::object time_range) {
           const py::list rs = py::module_::import("mad_icp_amd.records").attr("resolve_sources")(sources);
           std::vector<madicp_host::RecordSource> src(py::len(rs));
           std::vector<py::array> keep;  // (the buffers stay alive across the call)
           for (size_t k = 0; k < src.size(); ++k) {
             const py::tuple r = rs[k];
             keep.push_back(r[0].cast<py::array>());
             madicp_host::RecordSource& S = src[k];
             S.data = keep.back().data();
             S.n = r[1].cast<int64_t>();
             const py::tuple l = r[2];
             S.L = madicp_host::RecordLayout{l[0].cast<int32_t>(), l[1].cast<int32_t>(), l[2].cast<int32_t>(),
                                             l[3].cast<int32_t>(), l[4].cast<int32_t>(), l[5].cast<int32_t>()};
             const py::tuple R = r[3], t = r[4];
             for (int i = 0; i < 9; ++i) S.R[i] = R[i].cast<double>();
             for (int i = 0; i < 3; ++i) S.t[i] = t[i].cast<double>();
             S.min_range = r[5].cast<double>();
             S.max_range = r[6].cast<double>();
             S.t_scale = r[7].cast<double>();
             S.t_offset = r[8].cast<double>();
             S.kitti = r[9].cast<bool>() ? 1 : 0;
             const py::tuple a = r[10];
             S.A = madicp_host::AttrField{a[0].cast<int32_t>(), a[1].cast<int32_t>()};
           }
           double range[2];
           const bool have_range = !time_range.is_none();
           if (have_range) {
             const py::sequence tr = time_range.cast<py::sequence>();
             if (py::len(tr) != 2) throw py::value_error("time_range must be (t_begin, t_end)");
             range[0] = tr[0].cast<double>();
             range[1] = tr[1].cast<double>();
           }
           try {
             self.computeSourcesStamped(stamp, src.data(), static_cast<int>(src.size()), have_range ? range : nullptr);
           } catch (const std::invalid_argument& e) {
             throw py::value_error(e.what());
           }
         },
         py::arg("stamp"), py::arg("sources"), py::arg("time_range") = py::none())
    // additive: the keyframe map sharded over the ranks of a node (csrc/host/pipeline.h; mad_icp_amd.sharded.shard_pipeline
    // installs the communicator and calls this)
    .def("setShard", &Pipeline::setShard, py::arg("rank"), py::arg("world"))
    .def("shardRank", &Pipeline::shardRank)
    .def("shardWorld", &Pipeline::shardWorld)
    .def("numLocalKeyframes", &Pipeline::numLocalKeyframes)
    // instrumentation, not in the reference
    .def("lastInliersRatio", &Pipeline::lastInliersRatio)
    .def("lastRounds", &Pipeline::lastRounds)
#ifdef MADICP_MEASURE  // (test seam of the realtime budget rule: measurement build only)
    .def("setTimingForTest", &Pipeline::setTimingForTest, py::arg("pre_ms"), py::arg("round_ms"))
#endif
    .def("lastIcpMs", &Pipeline::lastIcpMs)
    .def("lastBuildMs", &Pipeline::lastBuildMs)
    .def("lastIcpPhasesMs", &Pipeline::lastIcpPhasesMs)
    .def("numKeyframes", &Pipeline::numKeyframes);
}
