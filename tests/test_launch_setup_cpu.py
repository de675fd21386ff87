"""The launchers' per-device setup (mmego_amd/csrc/launch_setup.h), on the CPU.

Structure: every dynamic-LDS limit and device query of mmego_amd/csrc goes through the header's helpers -- the HIP calls behind them
appear nowhere else, and no .hip file keeps a mutable static host variable (a per-process flag or cache) of its own.
Behaviour: the header is compiled as host C++ (g++) against a stand-in for the HIP runtime that records each call, with one current
device per thread as HIP keeps it."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mmego_amd", "csrc")
HEADER = "launch_setup.h"
SETUP_CALLS = re.compile(r"\b(hipFuncSetAttribute|hipDeviceGetAttribute|hipOccupancyMaxActiveBlocksPerMultiprocessor|hipGetDevice)\b")
# probe builds only (scripts/clock_probe.hip defines MMEGO_STAMP): the one static a .hip file may keep
STAMP_ONLY = {("lstm_step.hip", "mmego_step_dbg")}


def _code(name):
    """The file's text with comments blanked out (string literals kept)."""
    src = open(os.path.join(CSRC, name)).read()
    return re.sub(r'"(?:\\.|[^"\\\n])*"|//[^\n]*|/\*.*?\*/', lambda m: m.group(0) if m.group(0)[0] == '"' else " ", src, flags=re.S)


def _sources(ext):
    return sorted(f for f in os.listdir(CSRC) if f.endswith(ext))


def test_device_setup_calls_live_only_in_the_helper_header():
    assert HEADER in _sources(".h")
    found = {f: sorted(set(SETUP_CALLS.findall(_code(f)))) for f in _sources(".hip") + _sources(".h")}
    assert len(found[HEADER]) == 4, found[HEADER]
    assert {f: c for f, c in found.items() if c and f != HEADER} == {}


def _static_variables(code):
    """(name, offset) of each `static` declaration that is a variable: up to its first '=', ';', '[' or '{' with no '(' before."""
    for m in re.finditer(r"\bstatic\b([^;=\[{(]*)([;=\[{(])", code):
        if m.group(2) == "(":
            continue                                           # a function
        words = re.findall(r"\w+", m.group(1))
        if {"const", "constexpr", "__device__", "__constant__", "__shared__"} & set(words):
            continue
        yield words[-1], m.start()


def test_no_launcher_keeps_a_mutable_static():
    seen = set()
    for f in _sources(".hip"):
        code = _code(f)
        for name, at in _static_variables(code):
            assert (f, name) in STAMP_ONLY, "%s keeps the static %s" % (f, name)
            conds = re.findall(r"^\s*#\s*(if\w*\s+\w+|endif)", code[:at], flags=re.M)
            assert conds and conds[-1].split() == ["ifdef", "MMEGO_STAMP"], (f, name, conds[-3:])
            seen.add((f, name))
    assert seen == STAMP_ONLY
    # (the scan itself finds what it looks for)
    assert [n for n, _ in _static_variables("static bool a = false; static size_t b[64]; static int f(int); static const int c = 1;")] == ["a", "b"]


HIP_STANDIN = r"""
#pragma once
#include <chrono>
#include <cstddef>
#include <map>
#include <mutex>
#include <thread>
typedef int hipError_t;
enum { hipSuccess = 0, hipErrorInvalidValue = 1, hipErrorInvalidDevice = 101 };
enum hipFuncAttribute { hipFuncAttributeMaxDynamicSharedMemorySize };
enum hipDeviceAttribute_t { hipDeviceAttributeMultiprocessorCount };
thread_local int cur_dev = 0;                                  // HIP's current device: one per thread
int dev_err = hipSuccess, set_err = hipSuccess, sets = 0, cu_asks = 0, occ_asks = 0;
std::mutex rt;
std::map<std::pair<const void*, int>, int> held;               // (kernel, device) -> the limit HIP holds
hipError_t hipGetDevice(int* d) { *d = cur_dev; return dev_err; }
hipError_t hipFuncSetAttribute(const void* f, hipFuncAttribute, int v) {
  std::this_thread::sleep_for(std::chrono::microseconds(20));     // (a call that takes time: callers that race overlap in it)
  std::lock_guard<std::mutex> g(rt);
  if (set_err) return set_err;
  ++sets;
  held[{f, cur_dev}] = v;
  return hipSuccess;
}
hipError_t hipDeviceGetAttribute(int* v, hipDeviceAttribute_t, int dev) { ++cu_asks; *v = 200 + dev; return hipSuccess; }
template <class T> hipError_t hipOccupancyMaxActiveBlocksPerMultiprocessor(int* n, T, int block, size_t) { ++occ_asks; *n = 512 / block; return hipSuccess; }
"""

DRIVER = r"""
#include <cstdio>
#include <thread>
#include <vector>
#include "launch_setup.h"

void ka() {}
void kb() {}
void kc() {}
static int bad = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAIL line %d: %s\n", __LINE__, #c); ++bad; } } while (0)
static int held_for(void (*k)(), int dev) { std::lock_guard<std::mutex> g(rt); return held[{(const void*)k, dev}]; }

int main() {
  // per (kernel, device), raised only when the request exceeds what was set there
  CHECK(mmego_allow_lds<ka>(40000) == 0 && sets == 1 && held_for(ka, 0) == 40000);
  CHECK(mmego_allow_lds<ka>(30000) == 0 && mmego_allow_lds<ka>(40000) == 0 && mmego_allow_lds<ka>(0) == 0 && sets == 1);
  CHECK(mmego_allow_lds<kb>(30000) == 0 && sets == 2 && held_for(kb, 0) == 30000 && held_for(ka, 0) == 40000);
  cur_dev = 1;
  CHECK(mmego_allow_lds<ka>(30000) == 0 && sets == 3 && held_for(ka, 1) == 30000 && held_for(ka, 0) == 40000);
  cur_dev = 0;
  CHECK(mmego_allow_lds<ka>(150000) == 0 && sets == 4 && held_for(ka, 0) == 150000);
  // errors: HIP's, returned and not recorded (the next call asks again); one error for a device the tables cannot hold
  set_err = hipErrorInvalidValue;
  CHECK(mmego_allow_lds<kb>(200000) == hipErrorInvalidValue);
  set_err = hipSuccess;
  CHECK(mmego_allow_lds<kb>(100000) == 0 && sets == 5 && held_for(kb, 0) == 100000);
  for (int d : {-1, 64, 1000}) {
    cur_dev = d;
    CHECK(mmego_allow_lds<kb>(1) == hipErrorInvalidDevice && mmego_cu_count() == 0);
  }
  cur_dev = 0;
  dev_err = hipErrorInvalidDevice;
  CHECK(mmego_allow_lds<kc>(1) == hipErrorInvalidDevice && mmego_cu_count() == 0 && (mmego_resident_blocks<kc, 256>()) == 0);
  dev_err = hipSuccess;
  CHECK(sets == 5);
  // device queries: asked once per device
  CHECK(mmego_cu_count() == 200 && mmego_cu_count() == 200 && cu_asks == 1);
  cur_dev = 3;
  CHECK(mmego_cu_count() == 203 && cu_asks == 2);
  CHECK((mmego_resident_blocks<kc, 256>()) == 406 && (mmego_resident_blocks<kc, 256>()) == 406 && occ_asks == 1 && cu_asks == 2);
  cur_dev = 0;
  CHECK((mmego_resident_blocks<kc, 256>()) == 400 && (mmego_resident_blocks<kc, 128>()) == 800 && occ_asks == 3);
  // threads on two devices raising one kernel's limit at once: after each call HIP holds at least what was asked, and at the end
  // the largest request of each device (without the lock, a slower raise to a smaller limit lands last)
  std::vector<std::thread> ts;
  int low[8] = {};
  std::atomic<int> ready{0};
  for (int t = 0; t < 8; ++t)
    ts.emplace_back([t, &low, &ready] {
      cur_dev = 2 + (t & 1);
      for (++ready; ready < 8;) {}
      for (int i = 0; i < 4000; ++i) {
        const int want = 1 + 40 * i + 5 * t;
        if (mmego_allow_lds<kc>(want) != 0 || held_for(kc, cur_dev) < want) ++low[t];
      }
    });
  for (auto& t : ts) t.join();
  for (int t = 0; t < 8; ++t) CHECK(low[t] == 0);
  CHECK(held_for(kc, 2) == 1 + 40 * 3999 + 5 * 6 && held_for(kc, 3) == 1 + 40 * 3999 + 5 * 7);
  std::printf("bad %d\n", bad);
  return 0;
}
"""


def test_helper_keeps_each_limit_per_kernel_and_device(tmp_path):
    (tmp_path / "hip").mkdir()
    (tmp_path / "hip" / "hip_runtime.h").write_text(HIP_STANDIN)
    src, exe = tmp_path / "launch_setup.cpp", tmp_path / "launch_setup"
    src.write_text(DRIVER)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-pthread", "-I", str(tmp_path), "-I", CSRC, "-o", str(exe), str(src)],
                   check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True, timeout=120).stdout
    assert out.split()[-2:] == ["bad", "0"], out
