// _tbruntime: Python bindings for the MI355X-native actor-learner runtime.
//
// Python surface (capability parity with the reference's `libtorchbeast._C`
// module, ref: src/cc/libtorchbeast.cc + actorpool.cc:566-632 +
// rpcenv.cc:215-221): BatchingQueue, DynamicBatcher (+Batch), ActorPool,
// Server, exceptions ClosedBatchingQueue / AsyncError / NestError — plus the
// nest structural ops (map/map_many/map_many2/flatten/pack_as/front) that
// the reference ships as a separate `nest` extension.

#include <pybind11/functional.h>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>
#include <torch/extension.h>

#include <unistd.h>

#include <chrono>
#include <thread>

#include "actor_pool.h"
#include "env_server.h"
#include "inference_runner.h"
#include "nest.h"
#include "nest_pybind.h"
#include "queues.h"
#include "runtime_kernels.h"

namespace py = pybind11;
using namespace tbruntime;

namespace {

// ---------------------------------------------------------------------------
// GIL release for blocking calls made from daemon threads.
//
// Drivers run pool.run() and the batcher/queue iterators on daemon threads
// and exit while those threads unwind from the closed queues. A thread that
// asks for the GIL back once the interpreter is finalizing is ended by
// CPython with a forced stack unwind; through py::gil_scoped_release that
// unwind starts inside a destructor and std::terminate()s the process. Rows
// and mailboxes unwind the actor threads fast enough for a driver to reach
// finalization while its inference threads are still on their way out, so
// these entry points take the GIL back explicitly (outside any destructor,
// where pybind11 lets the forced unwind pass), and a thread that finds the
// interpreter already finalizing parks until the process exits.
// ---------------------------------------------------------------------------

inline bool python_finalizing() {
#if PY_VERSION_HEX >= 0x030D0000
  return Py_IsFinalizing() != 0;
#else
  return _Py_IsFinalizing() != 0;
#endif
}

class DaemonGilRelease {
 public:
  DaemonGilRelease() : state_(PyEval_SaveThread()) {}
  DaemonGilRelease(const DaemonGilRelease&) = delete;
  // For a consumer that found its queue closed and drained: the driver may
  // be about to exit, and a daemon thread that takes the GIL back now and
  // is still tearing down its Python frames (tensor deallocation drops and
  // retakes the GIL) when finalization starts dies the same way. Rows
  // withdraw queued requests on close, so a driver gets from close() to
  // exit in about a millisecond. Stay out of the interpreter for a short
  // grace period and park if it starts finalizing meanwhile.
  void linger_before_stop() {
    for (int i = 0; i < 10 && !python_finalizing(); ++i) {
      std::this_thread::sleep_for(std::chrono::milliseconds(5));
    }
  }
  void reacquire() {
    if (state_ == nullptr) return;
    if (python_finalizing()) park();
    PyThreadState* s = state_;
    state_ = nullptr;
    PyEval_RestoreThread(s);
  }
  // Exception path only (reacquire() was not reached).
  ~DaemonGilRelease() {
    if (state_ == nullptr) return;
    if (python_finalizing()) park();
    PyEval_RestoreThread(state_);
  }

 private:
  [[noreturn]] static void park() {
    for (;;) ::pause();
  }
  PyThreadState* state_;
};

// ---------------------------------------------------------------------------
// nest ops over arbitrary Python object trees.
// ---------------------------------------------------------------------------

bool is_container(const py::handle& h) {
  return py::isinstance<py::tuple>(h) || py::isinstance<py::list>(h) ||
         py::isinstance<py::dict>(h);
}

py::object nest_map(const py::function& f, const py::object& n) {
  if (py::isinstance<py::dict>(n)) {
    py::dict out;
    for (auto item : n.cast<py::dict>()) {
      out[item.first] = nest_map(f, py::reinterpret_borrow<py::object>(item.second));
    }
    return out;
  }
  if (py::isinstance<py::tuple>(n) || py::isinstance<py::list>(n)) {
    py::list out;
    for (auto item : n.cast<py::sequence>()) {
      out.append(nest_map(f, py::reinterpret_borrow<py::object>(item)));
    }
    if (py::isinstance<py::tuple>(n)) return py::tuple(out);
    return out;
  }
  return f(n);
}

void nest_flatten_into(const py::handle& n, py::list& out) {
  if (py::isinstance<py::dict>(n)) {
    py::list keys;
    for (auto item : n.cast<py::dict>()) keys.append(item.first);
    keys.attr("sort")();
    for (auto k : keys) nest_flatten_into(n.cast<py::dict>()[k], out);
  } else if (py::isinstance<py::tuple>(n) || py::isinstance<py::list>(n)) {
    for (auto item : n.cast<py::sequence>()) nest_flatten_into(item, out);
  } else {
    out.append(n);
  }
}

py::list nest_flatten(const py::object& n) {
  py::list out;
  nest_flatten_into(n, out);
  return out;
}

py::object nest_pack_as_impl(const py::handle& n, const py::list& flat,
                             size_t& pos) {
  if (py::isinstance<py::dict>(n)) {
    py::list keys;
    for (auto item : n.cast<py::dict>()) keys.append(item.first);
    keys.attr("sort")();
    py::dict filled;
    for (auto k : keys) {
      filled[k] = nest_pack_as_impl(n.cast<py::dict>()[k], flat, pos);
    }
    // Restore original key order.
    py::dict out;
    for (auto item : n.cast<py::dict>()) out[item.first] = filled[item.first];
    return out;
  }
  if (py::isinstance<py::tuple>(n) || py::isinstance<py::list>(n)) {
    py::list out;
    for (auto item : n.cast<py::sequence>()) {
      out.append(nest_pack_as_impl(item, flat, pos));
    }
    if (py::isinstance<py::tuple>(n)) return py::tuple(out);
    return out;
  }
  if (pos >= flat.size()) throw NestError("Too few elements to pack");
  return py::reinterpret_borrow<py::object>(flat[pos++]);
}

py::object nest_pack_as(const py::object& n, const py::list& flat) {
  size_t pos = 0;
  py::object out = nest_pack_as_impl(n, flat, pos);
  if (pos != flat.size()) throw NestError("Too many elements to pack");
  return out;
}

py::object nest_map_many(const py::function& f, const py::args& nests) {
  if (nests.size() == 0) throw NestError("map_many needs at least one nest");
  py::object first = nests[0];
  std::vector<py::list> flats;
  size_t n_leaves = 0;
  for (size_t i = 0; i < nests.size(); ++i) {
    flats.push_back(nest_flatten(nests[i]));
    if (i == 0) {
      n_leaves = flats[0].size();
    } else if (flats.back().size() != n_leaves) {
      throw NestError("nests don't match");
    }
  }
  py::list mapped;
  for (size_t leaf = 0; leaf < n_leaves; ++leaf) {
    py::list column;
    for (auto& fl : flats) column.append(fl[leaf]);
    mapped.append(f(column));
  }
  return nest_pack_as(first, mapped);
}

// unpack_rollouts_host() over tensors, same surface as the kernel's test
// binding: uint8 [outer, B, inner_bytes] outputs.
std::vector<torch::Tensor> unpack_rollouts_host_tensors(
    torch::Tensor staging, int64_t stride, int64_t B,
    std::vector<std::tuple<int64_t, int64_t, int64_t>> columns) {
  TORCH_CHECK(staging.device().is_cpu() &&
                  staging.scalar_type() == torch::kUInt8 &&
                  staging.is_contiguous(),
              "staging must be a contiguous uint8 CPU tensor");
  TORCH_CHECK(B >= 1 && stride >= 1 && staging.numel() >= B * stride,
              "staging smaller than B * stride");
  std::vector<torch::Tensor> out;
  std::vector<UnpackColumn> desc;
  for (const auto& c : columns) {
    const int64_t off = std::get<0>(c), outer = std::get<1>(c),
                  inner = std::get<2>(c);
    TORCH_CHECK(off >= 0 && outer >= 1 && inner >= 1 &&
                    off + outer * inner <= stride,
                "column overruns the staging row");
    out.push_back(torch::empty({outer, B, inner}, staging.options()));
    desc.push_back(
        UnpackColumn{off, inner, outer, out.back().data_ptr<uint8_t>()});
  }
  unpack_rollouts_host(staging.data_ptr<uint8_t>(), stride, B, desc.data(),
                       (int)desc.size());
  return out;
}

py::object nest_front(const py::object& n) {
  py::list flat = nest_flatten(n);
  if (flat.size() == 0) throw NestError("front() of empty nest");
  return py::reinterpret_borrow<py::object>(flat[0]);
}

}  // namespace

PYBIND11_MODULE(_tbruntime, m) {
  m.doc() = "MI355X-native torchbeast runtime (queues, actor pool, env server)";

  py::register_exception<ClosedQueue>(m, "ClosedBatchingQueue");
  py::register_exception<AsyncError>(m, "AsyncError");
  py::register_exception<NestError>(m, "NestError", PyExc_ValueError);

  // ---- nest ops ----
  m.def("map", &nest_map, py::arg("function"), py::arg("nest"));
  m.def("map_many", &nest_map_many, py::arg("function"));
  m.def(
      "map_many2",
      [](const py::function& f, const py::object& a, const py::object& b) {
        return nest_map_many(
            py::cpp_function([&f](const py::list& column) {
              return f(column[0], column[1]);
            }),
            py::make_tuple(a, b));
      },
      py::arg("function"), py::arg("nest1"), py::arg("nest2"));
  m.def("flatten", &nest_flatten, py::arg("nest"));
  m.def("pack_as", &nest_pack_as, py::arg("nest"), py::arg("sequence"));
  m.def("front", &nest_front, py::arg("nest"));

  // ---- rollout unpack kernel ----
  // GPU-output BatchingQueues reach the kernel through this hook (the
  // queue headers are also built into programs without any kernel).
  set_unpack_hook(&launch_unpack_rollouts);
  // Test-only: the kernel on a caller-made staging buffer; `columns` is a
  // list of (src_off, outer, inner_bytes).
  m.def("unpack_rollouts", &unpack_rollouts, py::arg("staging"),
        py::arg("stride"), py::arg("B"), py::arg("columns"));
  // Its oracle: the host reference unpack on a CPU staging tensor.
  m.def("unpack_rollouts_host", &unpack_rollouts_host_tensors,
        py::arg("staging"), py::arg("stride"), py::arg("B"),
        py::arg("columns"));

  // ---- inference-batch gather from rollout rows ----
  m.def("gather_rows_chunk_bytes", &gather_rows_chunk_bytes);
  // Test-only: the kernel over byte offsets into a pinned uint8 slab.
  m.def("gather_rows", &gather_rows, py::arg("slab"),
        py::arg("frame_offsets"), py::arg("reward_offsets"), py::arg("fsz"),
        py::arg("cap"), py::arg("chunk_bytes") = 0);
  // Test-only: build_row_table() over plain addresses (never dereferenced).
  // Returns (frame pointers, reward pointers, access width).
  m.def(
      "build_row_table",
      [](uint64_t slab_base, int64_t slab_bytes,
         std::vector<uint64_t> frame_addrs, std::vector<uint64_t> reward_addrs,
         int64_t fsz) {
        if (frame_addrs.size() != reward_addrs.size()) {
          throw std::invalid_argument("one reward address per frame address");
        }
        const int64_t b = (int64_t)frame_addrs.size();
        std::vector<const uint8_t*> ft(std::max<int64_t>(b, 1));
        std::vector<const float*> rt(std::max<int64_t>(b, 1));
        const unsigned width = build_row_table(
            b,
            [&](int64_t r) {
              return reinterpret_cast<const uint8_t*>(frame_addrs[r]);
            },
            [&](int64_t r) {
              return reinterpret_cast<const uint8_t*>(reward_addrs[r]);
            },
            fsz, reinterpret_cast<const uint8_t*>(slab_base), slab_bytes,
            ft.data(), rt.data());
        std::vector<uint64_t> fo(b), ro(b);
        for (int64_t r = 0; r < b; ++r) {
          fo[r] = reinterpret_cast<uintptr_t>(ft[r]);
          ro[r] = reinterpret_cast<uintptr_t>(rt[r]);
        }
        return std::make_tuple(fo, ro, width);
      },
      py::arg("slab_base"), py::arg("slab_bytes"), py::arg("frame_addrs"),
      py::arg("reward_addrs"), py::arg("fsz"));

  // ---- serve-plane heads and slot gather ----
  // Test-only: heads_sample_kernel on caller-made tensors, in both core
  // forms (rew = None: x alone), into caller-made pinned outputs.
  m.def("heads_sample", &heads_sample, py::arg("x"), py::arg("rew"),
        py::arg("policy_w"), py::arg("policy_b"), py::arg("base_w"),
        py::arg("base_b"), py::arg("b"), py::arg("greedy"), py::arg("seed"),
        py::arg("action"), py::arg("logits"), py::arg("baseline"));
  // Test-only: gather_obs_kernel as the runner calls it.
  m.def("gather_obs", &gather_obs, py::arg("slab_frames"),
        py::arg("slab_rew"), py::arg("slab_done"), py::arg("ids"),
        py::arg("bp"), py::arg("frame_shape"));

  // ---- LSTM serve step on state rows ----
  // Test-only: the layer kernels and the heads on caller-made tensors.
  m.def("lstm_serve_step", &lstm_serve_step, py::arg("x"), py::arg("rew"),
        py::arg("lstm_weights"), py::arg("policy_w"), py::arg("policy_b"),
        py::arg("base_w"), py::arg("base_b"), py::arg("state_block"),
        py::arg("in_offsets"), py::arg("out_offsets"), py::arg("done_slab"),
        py::arg("done_offsets"), py::arg("cap"), py::arg("greedy") = true,
        py::arg("seed") = 0);
  // Test-only: build_state_table() over plain addresses (never
  // dereferenced). Returns (state-in, state-out, done pointers).
  m.def(
      "build_state_table",
      [](uint64_t state_base, int64_t state_bytes, uint64_t slab_base,
         int64_t slab_bytes, std::vector<uint64_t> in_addrs,
         std::vector<uint64_t> out_addrs, std::vector<uint64_t> done_addrs,
         int64_t n_floats) {
        if (in_addrs.size() != out_addrs.size() ||
            in_addrs.size() != done_addrs.size()) {
          throw std::invalid_argument(
              "one state-out and one done address per state-in address");
        }
        const int64_t b = (int64_t)in_addrs.size();
        const size_t n = (size_t)std::max<int64_t>(b, 1);
        std::vector<const float*> it(n);
        std::vector<float*> ot(n);
        std::vector<const uint8_t*> dt(n);
        std::vector<uintptr_t> scratch;
        build_state_table(
            b,
            [&](int64_t r) {
              return reinterpret_cast<const uint8_t*>(in_addrs[r]);
            },
            [&](int64_t r) {
              return reinterpret_cast<const uint8_t*>(out_addrs[r]);
            },
            [&](int64_t r) {
              return reinterpret_cast<const uint8_t*>(done_addrs[r]);
            },
            n_floats, reinterpret_cast<const void*>(state_base), state_bytes,
            reinterpret_cast<const uint8_t*>(slab_base), slab_bytes, scratch,
            it.data(), ot.data(), dt.data());
        std::vector<uint64_t> io(b), oo(b), dd(b);
        for (int64_t r = 0; r < b; ++r) {
          io[r] = reinterpret_cast<uintptr_t>(it[r]);
          oo[r] = reinterpret_cast<uintptr_t>(ot[r]);
          dd[r] = reinterpret_cast<uintptr_t>(dt[r]);
        }
        return std::make_tuple(io, oo, dd);
      },
      py::arg("state_base"), py::arg("state_bytes"), py::arg("slab_base"),
      py::arg("slab_bytes"), py::arg("in_addrs"), py::arg("out_addrs"),
      py::arg("done_addrs"), py::arg("n_floats"));

  // ---- BatchingQueue ----
  py::class_<BatchingQueue, std::shared_ptr<BatchingQueue>>(m, "BatchingQueue")
      .def(py::init<int64_t, std::optional<int64_t>, std::optional<int64_t>,
                    std::optional<int64_t>, bool, std::optional<int64_t>,
                    std::optional<std::string>>(),
           py::arg("batch_dim") = 0,
           py::arg("minimum_batch_size") = std::nullopt,
           py::arg("maximum_batch_size") = std::nullopt,
           py::arg("timeout_ms") = std::nullopt,
           py::arg("check_inputs") = true,
           py::arg("maximum_queue_size") = std::nullopt,
           py::arg("output_device") = std::nullopt)
      .def_property_readonly("batch_dim", &BatchingQueue::batch_dim)
      .def("enqueue", &BatchingQueue::enqueue, py::arg("nest"),
           py::call_guard<py::gil_scoped_release>())
      .def("size", &BatchingQueue::size)
      .def("stats", &BatchingQueue::stats)
      .def("reset_stats", &BatchingQueue::reset_stats)
      .def("close", &BatchingQueue::close,
           py::call_guard<py::gil_scoped_release>())
      .def("is_closed", &BatchingQueue::is_closed)
      .def("__iter__", [](py::object self) { return self; })
      .def("__next__", [](BatchingQueue& q) {
        std::optional<TensorNest> batch;
        {
          DaemonGilRelease release;
          try {
            batch = q.dequeue_many().first;
          } catch (const ClosedQueue&) {
          }
          release.reacquire();
        }
        if (!batch) throw py::stop_iteration();
        return *batch;
      });

  // ---- DynamicBatcher ----
  auto batcher = py::class_<DynamicBatcher, std::shared_ptr<DynamicBatcher>>(
      m, "DynamicBatcher");

  py::class_<DynamicBatcher::Batch, std::shared_ptr<DynamicBatcher::Batch>>(
      batcher, "Batch")
      .def("get_inputs", &DynamicBatcher::Batch::get_inputs)
      .def("set_outputs", &DynamicBatcher::Batch::set_outputs,
           py::arg("outputs"))
      .def("size", &DynamicBatcher::Batch::size);

  batcher
      .def(py::init<int64_t, std::optional<int64_t>, std::optional<int64_t>,
                    std::optional<int64_t>, bool>(),
           py::arg("batch_dim") = 0,
           py::arg("minimum_batch_size") = std::nullopt,
           py::arg("maximum_batch_size") = std::nullopt,
           py::arg("timeout_ms") = std::nullopt,
           py::arg("check_outputs") = true)
      .def("compute", &DynamicBatcher::compute, py::arg("inputs"),
           py::call_guard<py::gil_scoped_release>())
      .def("size", &DynamicBatcher::size)
      .def("stats", &DynamicBatcher::stats)
      .def("reset_stats", &DynamicBatcher::reset_stats)
      .def("close", &DynamicBatcher::close,
           py::call_guard<py::gil_scoped_release>())
      .def("is_closed", &DynamicBatcher::is_closed)
      .def("__iter__", [](py::object self) { return self; })
      .def("__next__", [](DynamicBatcher& b) {
        std::shared_ptr<DynamicBatcher::Batch> batch;
        {
          DaemonGilRelease release;
          try {
            batch = b.get_batch();
          } catch (const ClosedQueue&) {
            release.linger_before_stop();
          }
          release.reacquire();
        }
        if (!batch) throw py::stop_iteration();
        return batch;
      });

  // ---- ActorPool ----
  py::class_<ActorPool, std::shared_ptr<ActorPool>>(m, "ActorPool")
      .def(py::init<int64_t, std::shared_ptr<BatchingQueue>,
                    std::shared_ptr<DynamicBatcher>, std::vector<std::string>,
                    TensorNest, int64_t, bool, int64_t, int64_t,
                    std::optional<bool>>(),
           py::arg("unroll_length"), py::arg("learner_queue"),
           py::arg("inference_batcher"), py::arg("env_server_addresses"),
           py::arg("initial_agent_state"), py::arg("seed_base") = 0,
           py::arg("use_obs_slab") = false,
           py::arg("rollout_budget_mb") = 0,
           py::arg("envs_per_thread") = 1,
           py::arg("recurrent_rows") = std::nullopt)
      .def("run",
           [](ActorPool& pool) {
             DaemonGilRelease release;
             pool.run();
             release.reacquire();
           })
      .def("obs_slab", &ActorPool::obs_slab,
           py::call_guard<py::gil_scoped_release>())
      .def("count", &ActorPool::count);

  // ---- InferenceRunner ----
  py::class_<InferenceRunner, std::shared_ptr<InferenceRunner>>(
      m, "InferenceRunner")
      .def(py::init<std::shared_ptr<DynamicBatcher>,
                    std::vector<torch::Tensor>, int64_t, bool, std::string>(),
           py::arg("inference_batcher"), py::arg("weights"),
           py::arg("num_lstm_layers") = 0, py::arg("greedy") = false,
           py::arg("model_type") = "shallow")
      .def("start", &InferenceRunner::start, py::arg("num_threads") = 2,
           py::call_guard<py::gil_scoped_release>())
      .def("stop", &InferenceRunner::stop,
           py::call_guard<py::gil_scoped_release>())
      .def("batches", &InferenceRunner::batches)
      .def("steps", &InferenceRunner::steps)
      .def("set_obs_slab", &InferenceRunner::set_obs_slab)
      .def("mark_weights_dirty", &InferenceRunner::mark_weights_dirty);

  // ---- EnvServer ----
  py::class_<EnvServer, std::shared_ptr<EnvServer>>(m, "Server")
      .def(py::init<py::object, std::string>(), py::arg("env_init"),
           py::arg("address"))
      .def("run", &EnvServer::run, py::call_guard<py::gil_scoped_release>())
      .def("start", &EnvServer::start)
      .def("stop", &EnvServer::stop,
           py::call_guard<py::gil_scoped_release>());
}
