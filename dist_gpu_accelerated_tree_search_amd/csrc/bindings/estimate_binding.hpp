// The dict both modules return for an indexed tree estimate (host twin in _tts_cpu, device
// estimator in _tts_hip): the TreeEstimate fields and, when asked, the per-probe records.
#pragma once

#include <pybind11/numpy.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include <cstring>
#include <string>

#include "../core/estimate.hpp"

namespace tts {

// method / power / look as both modules take them; anything unknown is a ValueError.
// look None: the model's own bound for lb 0/1, LB1 for lb 2 (an own-bound LB2 lookahead
// costs about 1 + k LB2 passes per level).
inline EstimateMethod parse_estimate_method(const std::string& method, int power, const pybind11::object& look, int lb) {
  EstimateMethod m;
  if (method == "lookahead")
    m.lookahead = true;
  else if (method != "knuth")
    throw std::invalid_argument("estimate method must be 'knuth' or 'lookahead', not '" + method + "'");
  if (power < 1 || power > kLookaheadMaxPower) throw std::invalid_argument("estimate power must be 1, 2 or 3");
  m.power = power;
  if (look.is_none()) {
    m.look = lb == 2 ? kLookBoundLb1 : kLookBoundOwn;
  } else {
    const std::string s = look.cast<std::string>();
    if (s == "own")
      m.look = kLookBoundOwn;
    else if (s == "lb1")
      m.look = kLookBoundLb1;
    else
      throw std::invalid_argument("estimate look must be 'own' or 'lb1', not '" + s + "'");
  }
  return m;
}

inline pybind11::dict estimate_dict(const TreeEstimate& e, const ProbeRecords* rec) {
  namespace py = pybind11;
  py::dict d;
  d["tree"] = e.tree;
  d["stderr"] = e.stderr_;
  d["depth"] = e.depth;
  d["probes"] = e.probes;
  d["per_level"] = e.per_level;
  if (rec) {
    const size_t n = rec->est.size();
    py::array_t<double> est(static_cast<py::ssize_t>(n));
    py::array_t<int> dep(static_cast<py::ssize_t>(n));
    py::array_t<int16_t> jobs({static_cast<py::ssize_t>(n), static_cast<py::ssize_t>(rec->jobs)});
    if (n) {
      std::memcpy(est.mutable_data(), rec->est.data(), n * sizeof(double));
      std::memcpy(dep.mutable_data(), rec->depth.data(), n * sizeof(int));
    }
    if (!rec->chosen.empty()) std::memcpy(jobs.mutable_data(), rec->chosen.data(), rec->chosen.size() * sizeof(int16_t));
    py::dict r;
    r["est"] = est;
    r["depth"] = dep;
    r["jobs"] = jobs;
    d["records"] = r;
  }
  return d;
}

}  // namespace tts
