// allsteps_abi.hip -- extern "C" implementation of include/allsteps.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/allsteps.h"
#include "allsteps_kernels.h"
#include "allsteps_events.h"
#include "allsteps_noise.h"
#include "allsteps_ray_camera.h"
#include "allsteps_ray_caster.h"

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

#define HIP_TRY(expr)                                                                        \
  do {                                                                                       \
    hipError_t _e = (expr);                                                                  \
    if (_e != hipSuccess) return fail(AS_ERR_HIP, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)

// STREAM-style copy: each thread moves 4 x 16 B per iteration (loads issued before stores), grid
// stride over the whole buffer, non-temporal so the copy does not thrash the MALL it measures past.
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
__global__ __launch_bounds__(256) void k_hbm_copy(u32x4* __restrict__ dst, const u32x4* __restrict__ src,
                                                   int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * 256 * 4;
  for (int64_t base = (int64_t)blockIdx.x * 256 * 4 + threadIdx.x; base < n; base += stride) {
    u32x4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (base + u * 256 < n) v[u] = __builtin_nontemporal_load(src + base + u * 256);
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (base + u * 256 < n) __builtin_nontemporal_store(v[u], dst + base + u * 256);
  }
}

}  // namespace

struct as_env {
  int32_t n;
  int32_t device;
  uint64_t seed;
  int64_t env_offset;
  as_state_t st;
  as::Consts* consts_dev;
  int32_t* counters_dev;  // two banks of kCntBank: step t uses bank t % 2, k_obs clears the other
  int32_t bank = 0, last_bank = 0;
  int32_t graph_safe = 0;  // as_set_graph_safe: fixed bank 0 + memset per call
  uint32_t* side_dev = nullptr;  // [kSideWords][n] k_step -> k_obs
  int32_t* wave_map_dev = nullptr;  // [n] cost-balanced placement (kMapEnvs), or null: xcd_block
  int32_t map_streamed = 0;         // k_step's grid is larger than the chip's workgroup slots
  bool sweep_skip = false;          // the model admits the compiled sweep skips (as_sweep_plan)
  int32_t num_steps;
  int32_t nv;
  as::Consts host;        // host copy of consts_dev (as_set_actuator / as_set_quad_task re-upload it)
  int32_t quad_ready = 0; // as_set_quad_task called
  // optional per-launch timing (as_profile): event triples around k_step / k_obs
  std::vector<hipEvent_t> ev;
  unsigned long long* stamps = nullptr;  // diagnostic (as_debug_stamps)
  as_contact_report_t report{};          // as_set_contact_report (count == nullptr: off)
  as::ReportDesc* report_dev = nullptr;  // its device copy, the block the launches point at
  const float* joint_cmd = nullptr;      // as_set_joint_commands (nullptr: off)
  int32_t prof_cap = 0, prof_n = 0, prof_stride = 1, prof_calls = 0;
};

extern "C" {

int as_abi_version(void) { return AS_ABI_VERSION; }

#ifndef AS_BUILD_ID
#define AS_BUILD_ID "unversioned"
#endif
const char* as_build_id(void) { return AS_BUILD_ID; }

int as_hbm_copy(void* dst, const void* src, int64_t n16, void* stream) {
  if (!dst || !src || n16 < 0) return fail(AS_ERR_INVALID, "as_hbm_copy: null pointer or negative size");
  if (((uintptr_t)dst | (uintptr_t)src) & 15) return fail(AS_ERR_INVALID, "as_hbm_copy: pointers must be 16-B aligned");
  if (n16 == 0) return AS_OK;
  const int64_t per_block = 256 * 4;
  const int64_t blocks = std::min<int64_t>((n16 + per_block - 1) / per_block, 1 << 20);
  hipLaunchKernelGGL(k_hbm_copy, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, (u32x4*)dst,
                     (const u32x4*)src, n16);
  HIP_TRY(hipGetLastError());
  return AS_OK;
}

const char* as_last_error(void) { return g_err.c_str(); }

int as_sweep_plan(const as_model_t* model, uint64_t* skip_mask) {
  if (!model) return fail(AS_ERR_INVALID, "as_sweep_plan: null model");
  std::string err;
  // no state here: foot ids 2 and 3 pass, as_create checks them against the state it is given
  if (!as::check_model(*model, true, err) || !as::check_parents(*model, err))
    return fail(AS_ERR_INVALID, "as_sweep_plan: " + err);
  const int nv = 6 + model->num_hinges;
  if (!as::step_supported_nv(nv)) return fail(AS_ERR_INVALID, "as_sweep_plan: no k_step instantiation for this model");
  const uint64_t valid = as::sweep_skip_mask(*model);
  const uint64_t compiled = nv == 27 ? as::kSweepSkip27 : as::kSweepSkip18;
  if (skip_mask) *skip_mask = valid;
  return (compiled & ~valid) == 0ull ? 1 : 0;
}

// as_create's last step: the handle's device memory and the uploads.  On an error the caller destroys env.
static int allocate_and_upload(as_env* env, const hipDeviceProp_t& prop) {
  const int num_envs = env->n;
  if (hipMalloc(&env->consts_dev, sizeof(as::Consts)) != hipSuccess ||
      hipMalloc(&env->counters_dev, 2 * as::kCntBank * sizeof(int32_t)) != hipSuccess ||
      hipMalloc(&env->side_dev, (size_t)as::kSideWords * num_envs * sizeof(uint32_t)) != hipSuccess ||
      hipMalloc(&env->report_dev, sizeof(as::ReportDesc)) != hipSuccess)
    return fail(AS_ERR_HIP, "as_create: hipMalloc failed");
  HIP_TRY(hipMemcpy(env->consts_dev, &env->host, sizeof(as::Consts), hipMemcpyHostToDevice));
  HIP_TRY(hipMemset(env->counters_dev, 0, 2 * as::kCntBank * sizeof(int32_t)));
  HIP_TRY(hipMemset(env->side_dev, 0, (size_t)as::kSideWords * num_envs * sizeof(uint32_t)));
  // cost-balanced placement (placement only: results are the same under any map); ALLSTEPS_WAVE_MAP=0
  // keeps the fixed XCD-contiguous placement (A/B timing)
  const char* wm = std::getenv("ALLSTEPS_WAVE_MAP");
  if (as::wave_map_fits(num_envs) && !(wm && std::strcmp(wm, "0") == 0)) {
    // k_step: one-wave workgroups of 2 envs, 8 per CU (LDS-bound, tests/kernel_budget.json)
    // (ALLSTEPS_WAVE_MAP=resident keeps the resident layout on a streamed grid: A/B timing)
    env->map_streamed = num_envs / 2 > 8 * prop.multiProcessorCount && !(wm && std::strcmp(wm, "resident") == 0);
    std::vector<int32_t> map((size_t)num_envs);  // the map k_obs builds from all-zero row counts (2 envs per workgroup)
    for (int w = 0; w < num_envs / as::kMapEnvs; ++w)
      for (int t = 0; t < as::kMapEnvs; ++t)
        map[(size_t)2 * as::wave_map_block(w, t >> 1, num_envs, env->map_streamed) + (t & 1)] = w * as::kMapEnvs + t;
    if (hipMalloc(&env->wave_map_dev, map.size() * sizeof(int32_t)) != hipSuccess)
      return fail(AS_ERR_HIP, "as_create: hipMalloc failed");
    HIP_TRY(hipMemcpy(env->wave_map_dev, map.data(), map.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  return AS_OK;
}

int as_create(int32_t num_envs, const as_model_t* model, const as_sim_t* sim, const as_task_t* task,
              const as_state_t* state, uint64_t seed, int32_t device, int64_t env_id_offset, as_env_t** out) {
  // 1. arguments
  if (!out || !model || !sim || !task || !state) return fail(AS_ERR_INVALID, "as_create: null argument");
  *out = nullptr;
  if (num_envs <= 0) return fail(AS_ERR_INVALID, "as_create: num_envs must be > 0");
  if (num_envs > AS_MAX_ENVS)
    return fail(AS_ERR_INVALID, "as_create: num_envs > AS_MAX_ENVS (" + std::to_string(AS_MAX_ENVS) +
                                    "): the kernels' state offsets are 32-bit; shard the envs over more handles");
  if (task->num_steps < 1 || task->num_steps > AS_NUM_STONES) return fail(AS_ERR_INVALID, "as_create: num_steps");
  if (sim->substeps < 1 || sim->pgs_iters < 0) return fail(AS_ERR_INVALID, "as_create: substeps/pgs_iters");
  const void* ptrs[] = {state->root_pos, state->root_quat, state->root_lin, state->root_ang, state->q,
                        state->qd, state->stones, state->pot, state->old_pot, state->foot_contact,
                        state->body_pos, state->idx, state->prev, state->next, state->count, state->swing,
                        state->ep_len, state->episode, state->contact_mask, state->curriculum};
  for (const void* p : ptrs)
    if (!p) return fail(AS_ERR_INVALID, "as_create: null state field");

  // 2. model
  std::string err;
  if (!as::check_model(*model, state->contact_mask_hind != nullptr, err)) return fail(AS_ERR_INVALID, "as_create: " + err);

  // 3. device
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(AS_ERR_NO_DEVICE, "as_create: no HIP device");
  if (device < 0 || device >= ndev) return fail(AS_ERR_INVALID, "as_create: bad device index");
  HIP_TRY(hipSetDevice(device));
  hipDeviceProp_t prop;
  HIP_TRY(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(AS_ERR_NO_DEVICE, std::string("as_create: device is ") + prop.gcnArchName + ", built for gfx950");

  // 4. plan: the constants block with the tree plan and the lane table
  as::Consts h{};
  h.model = *model;
  h.sim = *sim;
  h.task = *task;
  h.nv = 6 + model->num_hinges;
  h.act.mode = AS_ACT_TORQUE;
  h.st_has_hind = state->contact_mask_hind != nullptr;
  if (!as::plan_tree(h, err)) return fail(AS_ERR_INVALID, "as_create: " + err);
  if (!as::step_supported_nv(h.nv))
    return fail(AS_ERR_INVALID, "as_create: no k_step instantiation for " + std::to_string(h.nv) + " dofs");
  as::fill_lane_table(h);
  // collide pass B tests a stone pair on a group of up to 2^4 lanes (results are the same at any level);
  // ALLSTEPS_PAIR_GROUP=1..4 caps the level, 1 = one lane per pair throughout (tests, A/B timing)
  h.pair_group_cap = 4;
  if (const char* pg = std::getenv("ALLSTEPS_PAIR_GROUP")) {
    if (std::strlen(pg) != 1 || pg[0] < '1' || pg[0] > '4')
      return fail(AS_ERR_INVALID, std::string("as_create: ALLSTEPS_PAIR_GROUP=") + pg + ", expected 1, 2, 3 or 4");
    h.pair_group_cap = pg[0] - '0';
  }

  // 5. allocate and upload; past this point every failure destroys the handle
  as_env* env = new as_env();
  env->n = num_envs;
  env->device = device;
  env->seed = seed;
  env->env_offset = env_id_offset;
  env->st = *state;
  env->num_steps = task->num_steps;
  env->nv = h.nv;
  env->host = h;
  env->sweep_skip = as_sweep_plan(model, nullptr) == 1;
  const int rc = allocate_and_upload(env, prop);
  if (rc != AS_OK) {
    (void)as_destroy(env);
    return rc;
  }
  *out = env;
  return AS_OK;
}

int as_destroy(as_env_t* env) {
  if (!env) return AS_OK;
  (void)hipSetDevice(env->device);
  for (hipEvent_t e : env->ev) (void)hipEventDestroy(e);
  (void)hipFree(env->consts_dev);
  (void)hipFree(env->counters_dev);
  (void)hipFree(env->side_dev);
  (void)hipFree(env->wave_map_dev);
  (void)hipFree(env->report_dev);
  delete env;
  return AS_OK;
}

static int run(as_env_t* env, int mode, const float* actions, float* obs, float* reward, uint8_t* term,
               uint8_t* trunc, const float* reset_draws, void* stream, const uint8_t* reset_mask = nullptr) {
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  // no memset per step: this launch's counter bank was cleared by the previous launch's k_obs
  // (physics-only launches do not touch the counters and keep the bank)
  if (env->graph_safe && mode != as::kModePhysics) {
    env->bank = 0;
    // a kernel node, not hipMemsetAsync: replaying a captured memset node next to other graphs was
    // observed to leave the bank holding pointer-sized garbage on this ROCm build
    HIP_TRY(as::launch_zero(env->counters_dev, as::kCntBank, s));
  }
  int32_t* cnt = env->counters_dev + as::kCntBank * env->bank;
  as::StepArgs a{};
  a.consts = env->consts_dev;
  a.st = env->st;
  a.n = env->n;
  a.mode = mode;
  a.actions = actions;
  a.reward = reward;
  a.terminated = term;
  a.truncated = trunc;
  a.reset_draws = reset_draws;
  a.reset_mask = reset_mask;
  a.counters = cnt;
  a.seed = env->seed;
  a.env_offset = env->env_offset;
  a.stamps = env->stamps;
  a.obs = mode == as::kModePhysics ? nullptr : obs;
  a.side = env->side_dev;
  a.wave_map = env->wave_map_dev;
  a.rep = env->report.count ? env->report_dev : nullptr;
  // the joint commands serve the physics only: reset and task-only launches ignore them
  a.cmd = (mode == as::kModeStep || mode == as::kModePhysics) ? env->joint_cmd : nullptr;
  const bool prof = env->prof_n < env->prof_cap && (env->prof_calls++ % env->prof_stride) == 0;
  if (prof) HIP_TRY(hipEventRecord(env->ev[3 * env->prof_n], s));
  HIP_TRY(as::launch_step(a, env->nv, env->sweep_skip, s));
  if (prof) HIP_TRY(hipEventRecord(env->ev[3 * env->prof_n + 1], s));
  if (mode == as::kModePhysics) {
    if (prof) {
      HIP_TRY(hipEventRecord(env->ev[3 * env->prof_n + 2], s));
      ++env->prof_n;
    }
    return AS_OK;
  }
  as::ObsArgs o{};
  o.consts = env->consts_dev;
  o.st = env->st;
  o.n = env->n;
  o.counters = cnt;
  o.next_counters = env->counters_dev + as::kCntBank * (env->bank ^ 1);
  env->last_bank = env->bank;
  if (!env->graph_safe) env->bank ^= 1;
  o.obs = obs;
  o.side = env->side_dev;
  o.seed = env->seed;
  o.env_offset = env->env_offset;
  o.wave_map = env->wave_map_dev;
  o.map_streamed = env->map_streamed;
  HIP_TRY(as::launch_obs(o, s));
  if (prof) {
    HIP_TRY(hipEventRecord(env->ev[3 * env->prof_n + 2], s));
    ++env->prof_n;
  }
  return AS_OK;
}

int as_debug_stamps(as_env_t* env, uint64_t* stamps_dev) {
  if (!env) return fail(AS_ERR_INVALID, "as_debug_stamps: null handle");
  env->stamps = reinterpret_cast<unsigned long long*>(stamps_dev);
  return AS_OK;
}

int as_profile(as_env_t* env, int32_t max_launches) {
  if (!env || max_launches < 0) return fail(AS_ERR_INVALID, "as_profile: bad argument");
  HIP_TRY(hipSetDevice(env->device));
  for (hipEvent_t e : env->ev) HIP_TRY(hipEventDestroy(e));
  env->ev.assign(3 * (size_t)max_launches, nullptr);
  for (auto& e : env->ev) HIP_TRY(hipEventCreate(&e));
  env->prof_cap = max_launches;
  env->prof_n = 0;
  env->prof_stride = 1;
  env->prof_calls = 0;
  return AS_OK;
}

int as_profile_sampled(as_env_t* env, int32_t max_records, int32_t stride) {
  if (!env || stride < 1) return fail(AS_ERR_INVALID, "as_profile_sampled: bad argument");
  const int rc = as_profile(env, max_records);
  if (rc != AS_OK) return rc;
  env->prof_stride = stride;
  return AS_OK;
}

int as_profile_read(as_env_t* env, double* step_kernel_ms, double* obs_kernel_ms, int32_t* launches) {
  if (!env || !step_kernel_ms || !obs_kernel_ms || !launches) return fail(AS_ERR_INVALID, "as_profile_read: null");
  double a = 0.0, b = 0.0;
  if (env->prof_n > 0) HIP_TRY(hipEventSynchronize(env->ev[3 * env->prof_n - 1]));
  for (int i = 0; i < env->prof_n; ++i) {
    float t1 = 0.f, t2 = 0.f;
    HIP_TRY(hipEventElapsedTime(&t1, env->ev[3 * i], env->ev[3 * i + 1]));
    HIP_TRY(hipEventElapsedTime(&t2, env->ev[3 * i + 1], env->ev[3 * i + 2]));
    a += t1;
    b += t2;
  }
  *step_kernel_ms = a;
  *obs_kernel_ms = b;
  *launches = env->prof_n;
  env->prof_n = 0;
  return AS_OK;
}

int as_step(as_env_t* env, const float* actions, float* obs, float* reward, uint8_t* terminated, uint8_t* truncated,
            const float* reset_draws, void* stream) {
  if (!env || !actions || !obs || !reward || !terminated || !truncated)
    return fail(AS_ERR_INVALID, "as_step: null argument");
  return run(env, as::kModeStep, actions, obs, reward, terminated, truncated, reset_draws, stream);
}

int as_task_step(as_env_t* env, const float* actions, float* obs, float* reward, uint8_t* terminated,
                 uint8_t* truncated, const float* reset_draws, void* stream) {
  if (!env || !actions || !obs || !reward || !terminated || !truncated)
    return fail(AS_ERR_INVALID, "as_task_step: null argument");
  return run(env, as::kModeTask, actions, obs, reward, terminated, truncated, reset_draws, stream);
}

int as_set_seed(as_env_t* env, uint64_t seed) {
  if (!env) return fail(AS_ERR_INVALID, "as_set_seed: null handle");
  env->seed = seed;
  return AS_OK;
}

int as_reset_all(as_env_t* env, float* obs, const float* reset_draws, void* stream) {
  if (!env || !obs) return fail(AS_ERR_INVALID, "as_reset_all: null argument");
  return run(env, as::kModeReset, nullptr, obs, nullptr, nullptr, nullptr, reset_draws, stream);
}

int as_reset_mask(as_env_t* env, const uint8_t* mask, float* obs, const float* reset_draws, void* stream) {
  if (!env || !mask || !obs) return fail(AS_ERR_INVALID, "as_reset_mask: null argument");
  return run(env, as::kModeReset, nullptr, obs, nullptr, nullptr, nullptr, reset_draws, stream, mask);
}

int as_physics_step(as_env_t* env, const float* actions, void* stream) {
  if (!env || !actions) return fail(AS_ERR_INVALID, "as_physics_step: null argument");
  return run(env, as::kModePhysics, actions, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
}

// The setters' common end: env->host changed, so rebuild the lane table and replace the device block.
static int upload_consts(as_env_t* env) {
  as::fill_lane_table(env->host);
  // setup call, not stream-ordered: every launch still queued on any stream (torch's pool streams are
  // non-blocking, so a plain hipMemcpy would not wait for them) finishes before the block changes
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(env->consts_dev, &env->host, sizeof(as::Consts), hipMemcpyHostToDevice));
  return AS_OK;
}

int as_set_actuator(as_env_t* env, const as_actuator_t* act) {
  if (!env || !act) return fail(AS_ERR_INVALID, "as_set_actuator: null argument");
  if (act->mode != AS_ACT_TORQUE && act->mode != AS_ACT_DC_MOTOR) return fail(AS_ERR_INVALID, "as_set_actuator: mode");
  if (act->mode == AS_ACT_DC_MOTOR && !(act->velocity_limit > 0.f && act->effort_limit >= 0.f))
    return fail(AS_ERR_INVALID, "as_set_actuator: the DC motor needs velocity_limit > 0 and effort_limit >= 0");
  HIP_TRY(hipSetDevice(env->device));
  env->host.act = *act;
  return upload_consts(env);
}

int as_set_quad_task(as_env_t* env, const as_quad_task_t* q) {
  if (!env || !q) return fail(AS_ERR_INVALID, "as_set_quad_task: null argument");
  if (env->host.model.num_hinges != 12 || 28 + 3 * env->host.model.num_hinges != AS_QUAD_OBS_DIM)
    return fail(AS_ERR_INVALID, "as_set_quad_task: the task is defined for a 12-hinge quadruped");
  if (!env->st.contact_mask_hind || !env->st.feet)
    return fail(AS_ERR_INVALID, "as_set_quad_task: state->contact_mask_hind / state->feet is NULL");
  if (q->stop_frames < 1 || q->max_episode_length < 1 || !(q->step_dt > 0.f) || env->num_steps < 3 ||
      !(q->step_sigma > 0.f))
    return fail(AS_ERR_INVALID, "as_set_quad_task: stop_frames / max_episode_length / step_dt / num_steps / step_sigma");
  for (int f = 0; f < 4; ++f) {  // k_quad takes each swing foot's tip from its sensor geom
    bool found = false;
    for (int g = 0; g < env->host.model.num_geoms; ++g) found = found || env->host.model.geom_foot[g] == f;
    if (!found) return fail(AS_ERR_INVALID, "as_set_quad_task: the model needs a foot geom for each sensor 0..3");
  }
  HIP_TRY(hipSetDevice(env->device));
  env->host.quad = *q;
  const int rc = upload_consts(env);
  if (rc != AS_OK) return rc;
  env->quad_ready = 1;
  return AS_OK;
}

// reset_all with a mask: the masked reset (k_quad_reset_mask), which touches the masked envs only
static int quad(as_env_t* env, int reset_all, const float* actions, float* obs, float* reward, uint8_t* term,
                uint8_t* trunc, void* stream, const uint8_t* mask = nullptr) {
  if (!env->quad_ready) return fail(AS_ERR_INVALID, "as_quad_*: call as_set_quad_task first");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (!reset_all) {
    const int rc = run(env, as::kModePhysics, actions, nullptr, nullptr, nullptr, nullptr, nullptr, stream);
    if (rc != AS_OK) return rc;
  }
  as::QuadArgs a{};
  a.consts = env->consts_dev;
  a.st = env->st;
  a.n = env->n;
  a.reset_all = reset_all;
  a.actions = actions;
  a.obs = obs;
  a.reward = reward;
  a.terminated = term;
  a.truncated = trunc;
  a.seed = env->seed;
  a.env_offset = env->env_offset;
  a.side = env->side_dev;
  a.wave_map = env->wave_map_dev;
  a.map_streamed = env->map_streamed;
  a.rep = env->report.count ? env->report_dev : nullptr;
  if (mask) HIP_TRY(as::launch_quad_reset_mask(a, mask, s));
  else HIP_TRY(as::launch_quad(a, s));
  return AS_OK;
}

int as_quad_step(as_env_t* env, const float* actions, float* obs, float* reward, uint8_t* terminated,
                 uint8_t* truncated, void* stream) {
  if (!env || !actions || !obs || !reward || !terminated || !truncated)
    return fail(AS_ERR_INVALID, "as_quad_step: null argument");
  return quad(env, 0, actions, obs, reward, terminated, truncated, stream);
}

int as_quad_reset_all(as_env_t* env, float* obs, void* stream) {
  if (!env || !obs) return fail(AS_ERR_INVALID, "as_quad_reset_all: null argument");
  return quad(env, 1, nullptr, obs, nullptr, nullptr, nullptr, stream);
}

int as_quad_reset_mask(as_env_t* env, const uint8_t* mask, float* obs, void* stream) {
  if (!env || !mask || !obs) return fail(AS_ERR_INVALID, "as_quad_reset_mask: null argument");
  return quad(env, 1, nullptr, obs, nullptr, nullptr, nullptr, stream, mask);
}

int as_generate_stones(as_env_t* env, int32_t level, const float* draws, void* stream) {
  if (!env) return fail(AS_ERR_INVALID, "as_generate_stones: null handle");
  if (level < 0) return fail(AS_ERR_INVALID, "as_generate_stones: level < 0");
  as::StonesArgs a{};
  a.consts = env->consts_dev;
  a.stones = env->st.stones;
  a.n = env->n;
  a.level = level;
  a.draws = draws;
  a.seed = env->seed;
  a.env_offset = env->env_offset;
  HIP_TRY(as::launch_stones(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

int as_body_state(as_env_t* env, const as_body_table_t* bodies_host, float* out, void* stream) {
  if (!env || !bodies_host || !out) return fail(AS_ERR_INVALID, "as_body_state: null argument");
  const as_body_table_t& b = *bodies_host;
  if (b.num_bodies < 1 || b.num_bodies > AS_MAX_BODIES)
    return fail(AS_ERR_INVALID, "as_body_state: num_bodies out of range [1, AS_MAX_BODIES]");
  for (int i = 0; i < b.num_bodies; ++i)
    if (b.link[i] < 0 || b.link[i] >= env->host.model.num_links)
      return fail(AS_ERR_INVALID, "as_body_state: body link out of range");
  as::BodyArgs a{};
  a.consts = env->consts_dev;
  a.st = env->st;
  a.n = env->n;
  a.out = out;
  a.bodies = b;
  HIP_TRY(as::launch_body_state(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

int as_set_contact_report(as_env_t* env, const as_contact_report_t* report) {
  if (!env) return fail(AS_ERR_INVALID, "as_set_contact_report: null handle");
  if (!report) {
    env->report = as_contact_report_t{};
    return AS_OK;
  }
  if (!report->count || !report->records || !report->qd_prev)
    return fail(AS_ERR_INVALID, "as_set_contact_report: null buffer (count / records / qd_prev)");
  if (report->depth < 1 || report->depth > env->host.sim.substeps)
    return fail(AS_ERR_INVALID, "as_set_contact_report: depth " + std::to_string(report->depth) +
                                    " outside [1, sim.substeps = " + std::to_string(env->host.sim.substeps) + "]");
  // setup call, not stream-ordered (as upload_consts): queued launches finish before the block changes
  const as::ReportDesc d{report->count, report->records, report->qd_prev, report->depth};
  HIP_TRY(hipSetDevice(env->device));
  HIP_TRY(hipDeviceSynchronize());
  HIP_TRY(hipMemcpy(env->report_dev, &d, sizeof(d), hipMemcpyHostToDevice));
  env->report = *report;
  return AS_OK;
}

int as_set_joint_commands(as_env_t* env, const float* cmd_dev) {
  if (!env) return fail(AS_ERR_INVALID, "as_set_joint_commands: null handle");
  env->joint_cmd = cmd_dev;  // a launch argument: it holds from the next launch on
  return AS_OK;
}

int as_contact_forces(as_env_t* env, const as_body_table_t* bodies_host, float* force_matrix_out, float* net_out,
                      void* stream) {
  if (!env || !bodies_host || !force_matrix_out || !net_out)
    return fail(AS_ERR_INVALID, "as_contact_forces: null argument");
  if (!env->report.count) return fail(AS_ERR_INVALID, "as_contact_forces: no contact report set (as_set_contact_report)");
  const as_body_table_t& b = *bodies_host;
  if (b.num_bodies < 1 || b.num_bodies > AS_MAX_BODIES)
    return fail(AS_ERR_INVALID, "as_contact_forces: num_bodies out of range [1, AS_MAX_BODIES]");
  as::ForcesArgs a{};
  for (int i = 0; i < b.num_bodies; ++i) {
    if (b.link[i] < 0 || b.link[i] >= env->host.model.num_links)
      return fail(AS_ERR_INVALID, "as_contact_forces: body link out of range");
    a.link[i] = b.link[i];
  }
  a.n = env->n;
  a.depth = env->report.depth;
  a.count = env->report.count;
  a.records = env->report.records;
  a.matrix = force_matrix_out;
  a.net = net_out;
  a.num_bodies = b.num_bodies;
  HIP_TRY(as::launch_contact_forces(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

int as_contact_timers(as_env_t* env, const as_body_table_t* bodies_host, float* timers, float* timestamp,
                      float force_threshold, int32_t updates, const uint8_t* reset, const uint8_t* reset2,
                      void* stream) {
  if (!env || !bodies_host || !timers || !timestamp)
    return fail(AS_ERR_INVALID, "as_contact_timers: null argument (env / bodies / timers / timestamp)");
  if (!env->report.count) return fail(AS_ERR_INVALID, "as_contact_timers: no contact report set (as_set_contact_report)");
  if (updates != 0 && updates != env->report.depth)
    return fail(AS_ERR_INVALID, "as_contact_timers: updates " + std::to_string(updates) + " is neither 0 nor the " +
                                    "report's depth " + std::to_string(env->report.depth));
  if (!reset && reset2) return fail(AS_ERR_INVALID, "as_contact_timers: reset2 without reset");
  if (!(force_threshold >= 0.f) || !std::isfinite(force_threshold))
    return fail(AS_ERR_INVALID, "as_contact_timers: force_threshold " + std::to_string(force_threshold) +
                                    " is not a finite non-negative force");
  const as_body_table_t& b = *bodies_host;
  if (b.num_bodies < 1 || b.num_bodies > AS_MAX_BODIES)
    return fail(AS_ERR_INVALID, "as_contact_timers: num_bodies out of range [1, AS_MAX_BODIES]");
  as::TimersArgs a{};
  for (int i = 0; i < b.num_bodies; ++i) {
    if (b.link[i] < 0 || b.link[i] >= env->host.model.num_links)
      return fail(AS_ERR_INVALID, "as_contact_timers: body link out of range");
    a.link[i] = b.link[i];
  }
  a.n = env->n;
  a.updates = updates;
  a.count = env->report.count;
  a.records = env->report.records;
  a.timers = timers;
  a.timestamp = timestamp;
  a.reset = reset;
  a.reset2 = reset2;
  a.dt = env->host.sim.dt;
  a.force_threshold = force_threshold;
  a.num_bodies = b.num_bodies;
  HIP_TRY(as::launch_contact_timers(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

int as_ray_cast(as_env_t* env, const as_ray_caster_t* cfg_host, const float* rays, float* hits, int8_t* surface,
                float* pose, void* stream) {
  if (!env) return fail(AS_ERR_INVALID, "as_ray_cast: null argument env");
  if (!cfg_host) return fail(AS_ERR_INVALID, "as_ray_cast: null argument cfg");
  if (!rays) return fail(AS_ERR_INVALID, "as_ray_cast: null argument rays");
  if (!hits) return fail(AS_ERR_INVALID, "as_ray_cast: null argument hits");
  const as_ray_caster_t& c = *cfg_host;
  if (c.num_rays < 1 || c.num_rays > AS_MAX_RAYS)
    return fail(AS_ERR_INVALID, "as_ray_cast: num_rays " + std::to_string(c.num_rays) + " outside [1, AS_MAX_RAYS = " +
                                    std::to_string(AS_MAX_RAYS) + "]");
  if (c.surfaces == 0 || (c.surfaces & ~as::kRaySurfAll))
    return fail(AS_ERR_INVALID, "as_ray_cast: surfaces " + std::to_string(c.surfaces) +
                                    " is not AS_RAY_GROUND, AS_RAY_STONES or both");
  if (!std::isfinite(c.max_distance) || !(c.max_distance > 0.f))
    return fail(AS_ERR_INVALID, "as_ray_cast: max_distance " + std::to_string(c.max_distance) +
                                    " is not a finite positive distance");
  if (!std::isfinite(c.ground_z))
    return fail(AS_ERR_INVALID, "as_ray_cast: ground_z " + std::to_string(c.ground_z) + " is not finite");
  as::RayArgs a{};
  a.n = env->n;
  a.num_rays = c.num_rays;
  a.attach_yaw_only = c.attach_yaw_only != 0;
  a.surfaces = c.surfaces;
  a.num_steps = env->host.task.num_steps;
  a.max_distance = c.max_distance;
  a.ground_z = c.ground_z;
  for (int k = 0; k < 3; ++k) a.half[k] = env->host.sim.stone_half[k];
  a.root_pos = env->st.root_pos;
  a.root_quat = env->st.root_quat;
  a.stones = env->st.stones;
  a.rays = rays;
  a.hits = hits;
  a.surface = surface;
  a.pose = pose;
  HIP_TRY(as::launch_ray_cast(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

int as_ray_camera(as_env_t* env, const as_ray_camera_t* cfg_host, const float* dirs, const float* offset,
                  float* pose, float* plane, float* camera, float* normals, void* stream) {
  // (what needs no handle is checked first, the handle after)
  if (!cfg_host) return fail(AS_ERR_INVALID, "as_ray_camera: null argument cfg");
  if (!dirs) return fail(AS_ERR_INVALID, "as_ray_camera: null argument dirs");
  if (!offset) return fail(AS_ERR_INVALID, "as_ray_camera: null argument offset");
  if (!pose) return fail(AS_ERR_INVALID, "as_ray_camera: null argument pose");
  if (!plane && !camera && !normals)
    return fail(AS_ERR_INVALID, "as_ray_camera: plane, camera and normals are all null: no data type is requested");
  const as_ray_camera_t& c = *cfg_host;
  if (c.width < 1 || c.height < 1 || (int64_t)c.width * (int64_t)c.height > AS_MAX_CAMERA_RAYS)
    return fail(AS_ERR_INVALID, "as_ray_camera: image " + std::to_string(c.width) + " x " + std::to_string(c.height) +
                                    " is not positive with at most AS_MAX_CAMERA_RAYS = " +
                                    std::to_string(AS_MAX_CAMERA_RAYS) + " pixels");
  if (c.surfaces == 0 || (c.surfaces & ~as::kRaySurfAll))
    return fail(AS_ERR_INVALID, "as_ray_camera: surfaces " + std::to_string(c.surfaces) +
                                    " is not AS_RAY_GROUND, AS_RAY_STONES or both");
  if (c.clipping != AS_CAM_CLIP_NONE && c.clipping != AS_CAM_CLIP_MAX && c.clipping != AS_CAM_CLIP_ZERO)
    return fail(AS_ERR_INVALID, "as_ray_camera: clipping " + std::to_string(c.clipping) +
                                    " is not AS_CAM_CLIP_NONE, AS_CAM_CLIP_MAX or AS_CAM_CLIP_ZERO");
  if (!std::isfinite(c.max_distance) || !(c.max_distance > 0.f))
    return fail(AS_ERR_INVALID, "as_ray_camera: max_distance " + std::to_string(c.max_distance) +
                                    " is not a finite positive distance");
  if (!std::isfinite(c.ground_z))
    return fail(AS_ERR_INVALID, "as_ray_camera: ground_z " + std::to_string(c.ground_z) + " is not finite");
  if (!env) return fail(AS_ERR_INVALID, "as_ray_camera: null argument env");
  as::CamArgs a{};
  a.n = env->n;
  a.num_rays = c.width * c.height;
  a.surfaces = c.surfaces;
  a.clipping = c.clipping;
  a.num_steps = env->host.task.num_steps;
  a.max_distance = c.max_distance;
  a.ground_z = c.ground_z;
  for (int k = 0; k < 3; ++k) a.half[k] = env->host.sim.stone_half[k];
  a.root_pos = env->st.root_pos;
  a.root_quat = env->st.root_quat;
  a.stones = env->st.stones;
  a.dirs = dirs;
  a.offset = offset;
  a.pose = pose;
  a.plane = plane;
  a.camera = camera;
  a.normals = normals;
  HIP_TRY(as::launch_ray_camera(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

int as_imu(as_env_t* env, const as_imu_table_t* host, float dt, int all, uint8_t* outdated, float* data, float* prev,
           void* stream) {
  // (what needs no handle is checked first, the handle and what it sizes after)
  if (!host) return fail(AS_ERR_INVALID, "as_imu: null argument host");
  if (!outdated) return fail(AS_ERR_INVALID, "as_imu: null argument outdated");
  if (!data) return fail(AS_ERR_INVALID, "as_imu: null argument data");
  if (!prev) return fail(AS_ERR_INVALID, "as_imu: null argument prev");
  const as_imu_table_t& t = *host;
  if (t.num_sensors < 1 || t.num_sensors > AS_MAX_IMUS)
    return fail(AS_ERR_INVALID, "as_imu: num_sensors " + std::to_string(t.num_sensors) + " outside [1, AS_MAX_IMUS = " +
                                    std::to_string(AS_MAX_IMUS) + "]");
  if (!std::isfinite(dt) || !(dt > 0.f))
    return fail(AS_ERR_INVALID, "as_imu: dt " + std::to_string(dt) + " is not a finite positive time");
  if (!env) return fail(AS_ERR_INVALID, "as_imu: null argument env");
  for (int i = 0; i < t.num_sensors; ++i)
    if (t.link[i] < 0 || t.link[i] >= env->host.model.num_links)
      return fail(AS_ERR_INVALID, "as_imu: sensor " + std::to_string(i) + " link " + std::to_string(t.link[i]) +
                                      " outside the model's " + std::to_string(env->host.model.num_links) + " links");
  as::ImuArgs a{};
  a.consts = env->consts_dev;
  a.st = env->st;
  a.n = env->n;
  a.all = all != 0;
  a.dt = dt;
  a.outdated = outdated;
  a.data = data;
  a.prev = prev;
  a.imus = t;
  HIP_TRY(as::launch_imu(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

int as_frame_transformer(as_env_t* env, const as_frame_table_t* host, float* source, float* target, void* stream) {
  // (what needs no handle is checked first, the handle and what it sizes after)
  if (!host) return fail(AS_ERR_INVALID, "as_frame_transformer: null argument host");
  if (!source) return fail(AS_ERR_INVALID, "as_frame_transformer: null argument source");
  if (!target) return fail(AS_ERR_INVALID, "as_frame_transformer: null argument target");
  const as_frame_table_t& t = *host;
  const int S = t.num_sensors, F = t.num_frames;
  if (S < 1 || S > AS_MAX_FRAME_TRANSFORMERS)
    return fail(AS_ERR_INVALID, "as_frame_transformer: num_sensors " + std::to_string(S) +
                                    " outside [1, AS_MAX_FRAME_TRANSFORMERS = " +
                                    std::to_string(AS_MAX_FRAME_TRANSFORMERS) + "]");
  if (F < 1 || F > AS_MAX_FRAMES)
    return fail(AS_ERR_INVALID, "as_frame_transformer: num_frames " + std::to_string(F) +
                                    " outside [1, AS_MAX_FRAMES = " + std::to_string(AS_MAX_FRAMES) + "]");
  for (int f = 0; f < F; ++f) {
    const int s = t.sensor[f], before = f ? t.sensor[f - 1] : 0;
    if (s < 0 || s >= S)
      return fail(AS_ERR_INVALID, "as_frame_transformer: frame " + std::to_string(f) + " sensor " + std::to_string(s) +
                                      " outside [0, " + std::to_string(S) + ")");
    if ((f == 0 && s != 0) || s < before || s > before + 1 || (f == F - 1 && s != S - 1))
      return fail(AS_ERR_INVALID, "as_frame_transformer: frame " + std::to_string(f) + " sensor " + std::to_string(s) +
                                      " out of order: frames are grouped by sensor, every sensor has one");
  }
  if (!env) return fail(AS_ERR_INVALID, "as_frame_transformer: null argument env");
  const int links = env->host.model.num_links, stones = env->host.task.num_steps;
  for (int i = 0; i < S + F; ++i) {
    const as_frame_body_t& b = i < S ? t.source[i] : t.target[i - S];
    const std::string what = i < S ? "sensor " + std::to_string(i) + " source" : "frame " + std::to_string(i - S);
    if (b.link >= links)
      return fail(AS_ERR_INVALID, "as_frame_transformer: " + what + " link " + std::to_string(b.link) +
                                      " outside the model's " + std::to_string(links) + " links");
    if (b.link < 0 && (b.stone < 0 || b.stone >= stones))
      return fail(AS_ERR_INVALID, "as_frame_transformer: " + what + " stone " + std::to_string(b.stone) +
                                      " outside [0, num_steps = " + std::to_string(stones) + ")");
  }
  as::FrameTransformerArgs a{};
  a.consts = env->consts_dev;
  a.st = env->st;
  a.n = env->n;
  a.source = source;
  a.target = target;
  a.frames = t;
  HIP_TRY(as::launch_frame_transformer(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

// as_noise_*: a model's ranges and pointers.  `what` names the call and the model in the message.
static bool noise_model_ok(const as_noise_model_t& m, const std::string& what, std::string& err) {
  if (m.kind < AS_NOISE_CONSTANT || m.kind > AS_NOISE_GAUSSIAN)
    err = what + ": kind " + std::to_string(m.kind) + " outside AS_NOISE_CONSTANT .. AS_NOISE_GAUSSIAN";
  else if (m.op < AS_NOISE_ADD || m.op > AS_NOISE_ABS)
    err = what + ": op " + std::to_string(m.op) + " outside AS_NOISE_ADD .. AS_NOISE_ABS";
  else if (!m.p0 || (m.kind != AS_NOISE_CONSTANT && !m.p1))
    err = what + ": null parameter vector (p0 / p1)";
  else if (m.bias_kind < AS_NOISE_NONE || m.bias_kind > AS_NOISE_GAUSSIAN)
    err = what + ": bias_kind " + std::to_string(m.bias_kind) + " outside AS_NOISE_NONE .. AS_NOISE_GAUSSIAN";
  else if (m.bias_kind != AS_NOISE_NONE && (m.bias_op < AS_NOISE_ADD || m.bias_op > AS_NOISE_ABS))
    err = what + ": bias_op " + std::to_string(m.bias_op) + " outside AS_NOISE_ADD .. AS_NOISE_ABS";
  else if (m.bias_kind != AS_NOISE_NONE && !m.bias)
    err = what + ": null bias vector with a bias term";
  else
    return true;
  return false;
}

static bool noise_shape_ok(int32_t n, int32_t cols, const std::string& what, std::string& err) {
  if (n < 1 || n > AS_MAX_ENVS)
    err = what + ": n " + std::to_string(n) + " outside [1, AS_MAX_ENVS]";
  else if (cols < 1 || cols > as::kNoiseMaxCols)
    err = what + ": cols " + std::to_string(cols) + " outside [1, " + std::to_string(as::kNoiseMaxCols) +
          "]: a row's column quads must fit one wave";
  else
    return true;
  return false;
}

static int32_t noise_gshift(int cols) {
  int32_t s = 0;
  while ((1 << s) < as::noise_group(cols)) ++s;
  return s;
}

int as_noise_actions(const as_noise_model_t* model, const float* in, float* out, int32_t n, int32_t cols,
                     const uint32_t* t, const float* draws, uint64_t seed, int64_t env_id_offset, void* stream) {
  if (!model || !in || !out || !t) return fail(AS_ERR_INVALID, "as_noise_actions: null argument (model / in / out / t)");
  if (in == out) return fail(AS_ERR_INVALID, "as_noise_actions: out must not be in (out of place)");
  std::string err;
  if (!noise_shape_ok(n, cols, "as_noise_actions", err) || !noise_model_ok(*model, "as_noise_actions", err))
    return fail(AS_ERR_INVALID, err);
  as::NoiseActArgs a{};
  a.m = *model;
  a.in = in;
  a.out = out;
  a.n = n;
  a.cols = cols;
  a.gshift = noise_gshift(cols);
  a.t = t;
  a.draws = draws;
  a.seed = seed;
  a.env_offset = env_id_offset;
  HIP_TRY(as::launch_noise_actions(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

int as_noise_post(const as_noise_model_t* action_model, const as_noise_model_t* obs_model, float* obs, int32_t n,
                  int32_t cols, uint32_t* t, const uint8_t* reset, const uint8_t* reset2, const float* obs_draws,
                  const float* action_bias_draws, const float* obs_bias_draws, uint64_t seed,
                  int64_t env_id_offset, void* stream) {
  if (!t) return fail(AS_ERR_INVALID, "as_noise_post: null argument (t)");
  if (!reset && reset2) return fail(AS_ERR_INVALID, "as_noise_post: reset2 without reset");
  const bool apply = obs != nullptr && obs_model != nullptr;
  std::string err;
  if (!noise_shape_ok(n, apply ? cols : 1, "as_noise_post", err) ||
      (action_model && !noise_model_ok(*action_model, "as_noise_post: action model", err)) ||
      (obs_model && !noise_model_ok(*obs_model, "as_noise_post: observation model", err)))
    return fail(AS_ERR_INVALID, err);
  as::NoisePostArgs a{};
  if (action_model) a.act = *action_model;
  if (obs_model) a.obs = *obs_model;
  a.data = apply ? obs : nullptr;
  a.n = n;
  a.cols = apply ? cols : 0;
  a.gshift = noise_gshift(a.cols);
  a.t = t;
  a.reset = reset;
  a.reset2 = reset2;
  a.obs_draws = obs_draws;
  a.act_bias_draws = action_bias_draws;
  a.obs_bias_draws = obs_bias_draws;
  a.seed = seed;
  a.env_offset = env_id_offset;
  HIP_TRY(as::launch_noise_post(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

static bool events_shape_ok(int32_t num_terms, int32_t n, const std::string& what, std::string& err) {
  if (num_terms < 1 || num_terms > AS_MAX_EVENT_TERMS)
    err = what + ": num_terms " + std::to_string(num_terms) + " outside [1, AS_MAX_EVENT_TERMS = " +
          std::to_string(AS_MAX_EVENT_TERMS) + "]";
  else if (n < 1 || n > AS_MAX_ENVS)
    err = what + ": n " + std::to_string(n) + " outside [1, AS_MAX_ENVS]";
  else
    return true;
  return false;
}

int as_events_init(const as_event_term_t* terms, int32_t num_terms, float* time_left, uint32_t* t, int32_t n,
                   const float* interval_draws, uint64_t seed, int64_t env_id_offset, void* stream) {
  if (!terms || !time_left || !t) return fail(AS_ERR_INVALID, "as_events_init: null argument (terms / time_left / t)");
  std::string err;
  if (!events_shape_ok(num_terms, n, "as_events_init", err)) return fail(AS_ERR_INVALID, err);
  as::EventsArgs a{};
  a.terms = terms;
  a.num_terms = num_terms;
  a.n = n;
  a.time_left = time_left;
  a.t = t;
  a.interval_draws = interval_draws;
  a.seed = seed;
  a.env_offset = env_id_offset;
  HIP_TRY(as::launch_events_init(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

int as_events_interval(const as_event_term_t* terms, int32_t num_terms, float* root_lin, float* root_ang,
                       float* time_left, uint32_t* t, uint8_t* fired, int32_t n, float dt,
                       const float* interval_draws, const float* push_draws, uint64_t seed, int64_t env_id_offset,
                       void* stream) {
  if (!terms || !root_lin || !root_ang || !time_left || !t)
    return fail(AS_ERR_INVALID, "as_events_interval: null argument (terms / root_lin / root_ang / time_left / t)");
  std::string err;
  if (!events_shape_ok(num_terms, n, "as_events_interval", err)) return fail(AS_ERR_INVALID, err);
  if (!(dt > 0.f) || !std::isfinite(dt))
    return fail(AS_ERR_INVALID, "as_events_interval: dt " + std::to_string(dt) + " is not a positive finite step");
  as::EventsArgs a{};
  a.terms = terms;
  a.num_terms = num_terms;
  a.n = n;
  a.root_lin = root_lin;
  a.root_ang = root_ang;
  a.time_left = time_left;
  a.t = t;
  a.fired = fired;
  a.interval_draws = interval_draws;
  a.push_draws = push_draws;
  a.dt = dt;
  a.seed = seed;
  a.env_offset = env_id_offset;
  HIP_TRY(as::launch_events_interval(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

static bool commands_shape_ok(int32_t num_terms, int32_t n, const std::string& what, std::string& err) {
  if (num_terms < 1 || num_terms > AS_MAX_COMMAND_TERMS)
    err = what + ": num_terms " + std::to_string(num_terms) + " outside [1, AS_MAX_COMMAND_TERMS = " +
          std::to_string(AS_MAX_COMMAND_TERMS) + "]";
  else if (n < 1 || n > AS_MAX_ENVS)
    err = what + ": n " + std::to_string(n) + " outside [1, AS_MAX_ENVS]";
  else
    return true;
  return false;
}

int as_commands_step(const as_command_term_t* terms, int32_t num_terms, const float* root_quat,
                     const float* root_lin, const float* root_ang, float* vel, float* heading_target,
                     uint8_t* flags, float* time_left, int32_t* counter, float* metrics, float* last_metrics,
                     uint32_t* t, const uint8_t* reset, const uint8_t* reset2, int32_t n, float dt,
                     const float* draws, uint64_t seed, int64_t env_id_offset, void* stream) {
  if (!terms || !root_quat || !root_lin || !root_ang || !vel || !heading_target || !flags || !time_left || !counter ||
      !metrics || !t)
    return fail(AS_ERR_INVALID, "as_commands_step: null argument (terms / root_quat / root_lin / root_ang / vel / "
                                "heading_target / flags / time_left / counter / metrics / t)");
  std::string err;
  if (!commands_shape_ok(num_terms, n, "as_commands_step", err)) return fail(AS_ERR_INVALID, err);
  if (!(dt > 0.f) || !std::isfinite(dt))
    return fail(AS_ERR_INVALID, "as_commands_step: dt " + std::to_string(dt) + " is not a positive finite step");
  as::CommandsArgs a{};
  a.terms = terms;
  a.num_terms = num_terms;
  a.n = n;
  a.root_quat = root_quat;
  a.root_lin = root_lin;
  a.root_ang = root_ang;
  a.vel = vel;
  a.heading_target = heading_target;
  a.flags = flags;
  a.time_left = time_left;
  a.counter = counter;
  a.metrics = metrics;
  a.last_metrics = last_metrics;
  a.t = t;
  a.reset = reset;
  a.reset2 = reset2;
  a.draws = draws;
  a.dt = dt;
  a.seed = seed;
  a.env_offset = env_id_offset;
  HIP_TRY(as::launch_commands_step(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

int as_commands_reset(const as_command_term_t* terms, int32_t num_terms, float* vel, float* heading_target,
                      uint8_t* flags, float* time_left, int32_t* counter, float* metrics, float* last_metrics,
                      uint32_t* t, const uint8_t* mask, int32_t n, const float* draws, uint64_t seed,
                      int64_t env_id_offset, void* stream) {
  if (!terms || !vel || !heading_target || !flags || !time_left || !counter || !metrics || !t)
    return fail(AS_ERR_INVALID, "as_commands_reset: null argument (terms / vel / heading_target / flags / time_left / "
                                "counter / metrics / t)");
  std::string err;
  if (!commands_shape_ok(num_terms, n, "as_commands_reset", err)) return fail(AS_ERR_INVALID, err);
  as::CommandsArgs a{};
  a.terms = terms;
  a.num_terms = num_terms;
  a.n = n;
  a.vel = vel;
  a.heading_target = heading_target;
  a.flags = flags;
  a.time_left = time_left;
  a.counter = counter;
  a.metrics = metrics;
  a.last_metrics = last_metrics;
  a.t = t;
  a.reset = mask;
  a.draws = draws;
  a.seed = seed;
  a.env_offset = env_id_offset;
  HIP_TRY(as::launch_commands_reset(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

int as_observations_step(const as_observation_term_t* terms, int32_t num_terms, const float* cols,
                         const int32_t* omap, int32_t d0, int32_t out_cols, int32_t group,
                         const as_observation_sources_t* sources, float* out, int32_t* count, uint32_t* t,
                         const uint8_t* reset, const uint8_t* reset2, int32_t n, const float* draws, uint64_t seed,
                         int64_t env_id_offset, void* stream) {
  if (!terms || !cols || !omap || !sources || !out || !count || !t)
    return fail(AS_ERR_INVALID, "as_observations_step: null argument (terms / cols / omap / sources / out / count / "
                                "t)");
  if (num_terms < 1 || num_terms > AS_MAX_OBS_TERMS)
    return fail(AS_ERR_INVALID, "as_observations_step: num_terms " + std::to_string(num_terms) +
                                    " outside [1, AS_MAX_OBS_TERMS = " + std::to_string(AS_MAX_OBS_TERMS) + "]");
  if (d0 < 1 || d0 > AS_MAX_OBS_COLS || out_cols < d0 || out_cols > AS_MAX_OBS_OUT_COLS)
    return fail(AS_ERR_INVALID, "as_observations_step: " + std::to_string(d0) + " columns (at most AS_MAX_OBS_COLS = " +
                                    std::to_string(AS_MAX_OBS_COLS) + "), " + std::to_string(out_cols) +
                                    " with history (at most AS_MAX_OBS_OUT_COLS = " +
                                    std::to_string(AS_MAX_OBS_OUT_COLS) + ")");
  if (group < 0 || group >= AS_MAX_OBS_GROUPS)
    return fail(AS_ERR_INVALID, "as_observations_step: group " + std::to_string(group) +
                                    " outside [0, AS_MAX_OBS_GROUPS)");
  if (n < 1 || n > AS_MAX_ENVS) return fail(AS_ERR_INVALID, "as_observations_step: n outside [1, AS_MAX_ENVS]");
  for (int s = 0; s < AS_OBS_NUM_SOURCES; ++s)
    if (sources->rows[s] < 0 || (sources->ptr[s] && sources->rows[s] < 1))
      return fail(AS_ERR_INVALID, "as_observations_step: source " + std::to_string(s) + " has no rows");
  as::ObservationsArgs a{};
  a.terms = terms;
  a.cols = cols;
  a.omap = omap;
  a.num_terms = num_terms;
  a.d0 = d0;
  a.out_cols = out_cols;
  a.group = group;
  a.n = n;
  a.src = *sources;
  a.out = out;
  a.count = count;
  a.t = t;
  a.reset = reset;
  a.reset2 = reset2;
  a.draws = draws;
  a.seed = seed;
  a.env_offset = env_id_offset;
  HIP_TRY(as::launch_observations(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

int as_observations_reset(float* out, int32_t out_cols, int32_t* count, const uint8_t* mask, int32_t n,
                          void* stream) {
  if (!out || !count) return fail(AS_ERR_INVALID, "as_observations_reset: null argument (out / count)");
  if (out_cols < 1 || out_cols > AS_MAX_OBS_OUT_COLS)
    return fail(AS_ERR_INVALID, "as_observations_reset: out_cols " + std::to_string(out_cols) +
                                    " outside [1, AS_MAX_OBS_OUT_COLS]");
  if (n < 1 || n > AS_MAX_ENVS) return fail(AS_ERR_INVALID, "as_observations_reset: n outside [1, AS_MAX_ENVS]");
  as::ObservationsArgs a{};
  a.out = out;
  a.out_cols = out_cols;
  a.count = count;
  a.reset = mask;
  a.n = n;
  HIP_TRY(as::launch_observations_reset(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

int as_rewards_step(const as_reward_term_t* terms, int32_t num_terms, const float* table, uint32_t kinds,
                    const as_reward_sources_t* sources, float* reward, float* episode_sums, float* step_reward,
                    float* last_episode_sums, float* prev_actions, const uint8_t* reset, const uint8_t* reset2,
                    int32_t n, float dt, void* stream) {
  if (!terms || !table || !sources || !reward || !episode_sums || !step_reward)
    return fail(AS_ERR_INVALID, "as_rewards_step: null argument (terms / table / sources / reward / episode_sums / "
                                "step_reward)");
  if (num_terms < 1 || num_terms > AS_MAX_REW_TERMS)
    return fail(AS_ERR_INVALID, "as_rewards_step: num_terms " + std::to_string(num_terms) +
                                    " outside [1, AS_MAX_REW_TERMS = " + std::to_string(AS_MAX_REW_TERMS) + "]");
  if (n < 1 || n > AS_MAX_ENVS) return fail(AS_ERR_INVALID, "as_rewards_step: n outside [1, AS_MAX_ENVS]");
  if (!std::isfinite(dt) || dt <= 0.0f) return fail(AS_ERR_INVALID, "as_rewards_step: dt is not finite or <= 0");
  if (kinds >> AS_REW_NUM_KINDS) return fail(AS_ERR_INVALID, "as_rewards_step: kinds has bits of unknown kinds");
  const as_reward_sources_t& S = *sources;
  auto bit = [&](int k) { return ((kinds >> k) & 1u) != 0; };
  auto missing = [&](int k, const char* what) {
    return fail(AS_ERR_INVALID, std::string("as_rewards_step: a term of kind ") + std::to_string(k) +
                                    " needs the source " + what + ", which is NULL or has no rows");
  };
  const bool root_state = S.root_quat && S.root_lin && S.root_ang;
  const bool sim_dt = std::isfinite(S.sim_dt) && S.sim_dt > 0.0f;
  const bool cmds = S.commands && S.command_rows >= 3;
  const bool joints = S.q && S.qd && S.joint_rows >= 1;
  const bool acts = S.actions && S.action_cols >= 1;
  const bool net = S.net && S.depth >= 1 && S.bodies >= 1 && sim_dt;
  const bool timers = S.timers && S.timer_bodies >= 1;
  for (int k = 0; k < AS_REW_NUM_KINDS; ++k) {
    if (!bit(k)) continue;
    switch (k) {
      case AS_REW_IS_ALIVE: case AS_REW_IS_TERMINATED:
        if (!S.terminated) return missing(k, "terminated");
        break;
      case AS_REW_LIN_VEL_Z_L2: case AS_REW_ANG_VEL_XY_L2: case AS_REW_FLAT_ORIENTATION_L2:
        if (!root_state) return missing(k, "root_quat / root_lin / root_ang");
        break;
      case AS_REW_BASE_HEIGHT_L2:
        if (!S.root_pos) return missing(k, "root_pos");
        break;
      case AS_REW_JOINT_VEL_L1: case AS_REW_JOINT_VEL_L2: case AS_REW_JOINT_DEVIATION_L1:
      case AS_REW_JOINT_POS_LIMITS:
        if (!joints) return missing(k, "q / qd");
        break;
      case AS_REW_JOINT_ACC_L2:
        if (!joints || !S.qd_prev || S.qd_prev_rows < 1 || !sim_dt) return missing(k, "qd_prev (and sim_dt)");
        break;
      case AS_REW_ACTION_L2:
        if (!acts) return missing(k, "actions");
        break;
      case AS_REW_ACTION_RATE_L2:
        if (!acts || !prev_actions) return missing(k, "actions / prev_actions");
        break;
      case AS_REW_UNDESIRED_CONTACTS: case AS_REW_CONTACT_FORCES:
        if (!net) return missing(k, "net (and sim_dt)");
        break;
      case AS_REW_FEET_AIR_TIME: case AS_REW_FEET_AIR_TIME_BIPED:
        if (!timers || !cmds) return missing(k, "timers / commands");
        break;
      case AS_REW_TRACK_LIN_VEL_XY_EXP: case AS_REW_TRACK_ANG_VEL_Z_EXP: case AS_REW_TRACK_LIN_VEL_XY_YAW_EXP:
        if (!root_state || !cmds) return missing(k, "root state / commands");
        break;
      case AS_REW_TRACK_ANG_VEL_Z_WORLD_EXP:
        if (!S.root_ang || !cmds) return missing(k, "root_ang / commands");
        break;
    }
  }
  if (prev_actions && !acts)
    return fail(AS_ERR_INVALID, "as_rewards_step: prev_actions without actions (NULL, or no columns)");
  if (S.joint_rows < 0 || S.qd_prev_rows < 0 || S.command_rows < 0 || S.depth < 0 || S.bodies < 0 ||
      S.timer_bodies < 0 || S.action_cols < 0 || (prev_actions && S.actions && S.action_cols < 1))
    return fail(AS_ERR_INVALID, "as_rewards_step: a negative row count, or actions without columns");
  as::RewardsArgs a{};
  a.terms = terms;
  a.table = table;
  a.num_terms = num_terms;
  a.n = n;
  a.src = S;
  a.reward = reward;
  a.episode_sums = episode_sums;
  a.step_reward = step_reward;
  a.last_episode_sums = last_episode_sums;
  a.prev_actions = prev_actions;
  a.reset = reset;
  a.reset2 = reset2;
  a.dt = dt;
  HIP_TRY(as::launch_rewards_step(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

int as_rewards_reset(float* episode_sums, int32_t num_terms, float* prev_actions, int32_t action_cols,
                     const uint8_t* mask, int32_t n, void* stream) {
  if (!episode_sums) return fail(AS_ERR_INVALID, "as_rewards_reset: null argument (episode_sums)");
  if (num_terms < 1 || num_terms > AS_MAX_REW_TERMS)
    return fail(AS_ERR_INVALID, "as_rewards_reset: num_terms outside [1, AS_MAX_REW_TERMS]");
  if (prev_actions && action_cols < 1) return fail(AS_ERR_INVALID, "as_rewards_reset: prev_actions without columns");
  if (n < 1 || n > AS_MAX_ENVS) return fail(AS_ERR_INVALID, "as_rewards_reset: n outside [1, AS_MAX_ENVS]");
  as::RewardsArgs a{};
  a.episode_sums = episode_sums;
  a.num_terms = num_terms;
  a.prev_actions = prev_actions;
  a.src.action_cols = action_cols;
  a.reset = mask;
  a.n = n;
  HIP_TRY(as::launch_rewards_reset(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

int as_terminations_step(const as_termination_term_t* terms, int32_t num_terms, const float* table, uint32_t kinds,
                         const as_termination_sources_t* sources, uint8_t* term_dones, uint8_t* time_outs,
                         uint8_t* terminated, uint8_t* dones, uint8_t* last_episode_dones, uint8_t* reset_request,
                         int32_t n, void* stream) {
  if (!terms || !table || !sources || !term_dones || !time_outs || !terminated || !dones)
    return fail(AS_ERR_INVALID, "as_terminations_step: null argument (terms / table / sources / term_dones / "
                                "time_outs / terminated / dones)");
  if (num_terms < 1 || num_terms > AS_MAX_TERMINATION_TERMS)
    return fail(AS_ERR_INVALID, "as_terminations_step: num_terms " + std::to_string(num_terms) +
                                    " outside [1, AS_MAX_TERMINATION_TERMS = " +
                                    std::to_string(AS_MAX_TERMINATION_TERMS) + "]");
  if (n < 1 || n > AS_MAX_ENVS) return fail(AS_ERR_INVALID, "as_terminations_step: n outside [1, AS_MAX_ENVS]");
  if (kinds >> AS_TERMINATION_NUM_KINDS)
    return fail(AS_ERR_INVALID, "as_terminations_step: kinds has bits of unknown kinds");
  const as_termination_sources_t& S = *sources;
  if (S.joint_rows < 0 || S.command_terms < 0 || S.depth < 0 || S.bodies < 0)
    return fail(AS_ERR_INVALID, "as_terminations_step: a negative row count");
  auto missing = [&](int k, const char* what) {
    return fail(AS_ERR_INVALID, std::string("as_terminations_step: a term of kind ") + std::to_string(k) +
                                    " needs the source " + what + ", which is NULL or has no rows");
  };
  for (int k = 0; k < AS_TERMINATION_NUM_KINDS; ++k) {
    if (!((kinds >> k) & 1u)) continue;
    switch (k) {
      case AS_TERMINATION_TIME_OUT:
        if (!S.ep_len) return missing(k, "ep_len");
        break;
      case AS_TERMINATION_COMMAND_RESAMPLE:
        if (!S.time_left || !S.command_counter || S.command_terms < 1)
          return missing(k, "time_left / command_counter");
        break;
      case AS_TERMINATION_BAD_ORIENTATION:
        if (!S.root_quat) return missing(k, "root_quat");
        break;
      case AS_TERMINATION_ROOT_HEIGHT_BELOW_MINIMUM:
        if (!S.root_pos) return missing(k, "root_pos");
        break;
      case AS_TERMINATION_JOINT_POS_OUT_OF_LIMIT: case AS_TERMINATION_JOINT_POS_OUT_OF_MANUAL_LIMIT:
        if (!S.q || S.joint_rows < 1) return missing(k, "q");
        break;
      case AS_TERMINATION_JOINT_VEL_OUT_OF_MANUAL_LIMIT:
        if (!S.qd || S.joint_rows < 1) return missing(k, "qd");
        break;
      case AS_TERMINATION_ILLEGAL_CONTACT:
        if (!S.net || S.depth < 1 || S.bodies < 1 || !std::isfinite(S.sim_dt) || !(S.sim_dt > 0.0f))
          return missing(k, "net (and sim_dt)");
        break;
    }
  }
  as::TerminationsArgs a{};
  a.terms = terms;
  a.table = table;
  a.num_terms = num_terms;
  a.n = n;
  a.src = S;
  a.term_dones = term_dones;
  a.time_outs = time_outs;
  a.terminated = terminated;
  a.dones = dones;
  a.last_episode_dones = last_episode_dones;
  a.reset_request = reset_request;
  HIP_TRY(as::launch_terminations_step(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

static int actions_check(const char* who, const as_action_column_t* cols, int32_t num_cols, int32_t cmd_cols,
                         int32_t n) {
  if (!cols) return fail(AS_ERR_INVALID, std::string(who) + ": null cols");
  if (num_cols < 1 || num_cols > AS_ACT_DIM)
    return fail(AS_ERR_INVALID, std::string(who) + ": num_cols " + std::to_string(num_cols) +
                                    " outside [1, AS_ACT_DIM = " + std::to_string(AS_ACT_DIM) + "]");
  if (cmd_cols < 1 || cmd_cols > AS_ACT_DIM)
    return fail(AS_ERR_INVALID, std::string(who) + ": joint count " + std::to_string(cmd_cols) +
                                    " outside [1, AS_ACT_DIM = " + std::to_string(AS_ACT_DIM) + "]");
  if (n < 1 || n > AS_MAX_ENVS) return fail(AS_ERR_INVALID, std::string(who) + ": n outside [1, AS_MAX_ENVS]");
  return AS_OK;
}

int as_actions_step(const as_action_column_t* cols, int32_t num_cols, const float* input, float* action,
                    float* prev_action, float* processed, float* prev_applied, float* cmd, int32_t cmd_cols,
                    int32_t n, void* stream) {
  const int rc = actions_check("as_actions_step", cols, num_cols, cmd_cols, n);
  if (rc != AS_OK) return rc;
  if (!input || !action || !prev_action || !processed || !prev_applied || !cmd)
    return fail(AS_ERR_INVALID, "as_actions_step: null argument (input / action / prev_action / processed / "
                                "prev_applied / cmd)");
  as::ActionsArgs a{};
  a.cols = cols;
  a.num_cols = num_cols;
  a.cmd_cols = cmd_cols;
  a.n = n;
  a.input = input;
  a.action = action;
  a.prev_action = prev_action;
  a.processed = processed;
  a.prev_applied = prev_applied;
  a.cmd = cmd;
  HIP_TRY(as::launch_actions_process(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

int as_actions_reset(const as_action_column_t* cols, int32_t num_cols, float* action, float* prev_action,
                     float* prev_applied, const float* q, int32_t q_rows, const uint8_t* mask, const uint8_t* mask2,
                     int32_t n, void* stream) {
  const int rc = actions_check("as_actions_reset", cols, num_cols, q_rows, n);
  if (rc != AS_OK) return rc;
  if (!action || !prev_action || !prev_applied || !q)
    return fail(AS_ERR_INVALID, "as_actions_reset: null argument (action / prev_action / prev_applied / q)");
  as::ActionsArgs a{};
  a.cols = cols;
  a.num_cols = num_cols;
  a.cmd_cols = q_rows;
  a.n = n;
  a.action = action;
  a.prev_action = prev_action;
  a.prev_applied = prev_applied;
  a.q = q;
  a.mask = mask;
  a.mask2 = mask2;
  HIP_TRY(as::launch_actions_reset(a, reinterpret_cast<hipStream_t>(stream)));
  return AS_OK;
}

int as_set_graph_safe(as_env_t* env, int32_t on) {
  if (!env) return fail(AS_ERR_INVALID, "as_set_graph_safe: null handle");
  env->graph_safe = on != 0;
  return AS_OK;
}

int as_step_counters(as_env_t* env, const int32_t** counters_dev) {
  if (!env || !counters_dev) return fail(AS_ERR_INVALID, "as_step_counters: null argument");
  *counters_dev = env->counters_dev + as::kCntBank * env->last_bank;
  return AS_OK;
}

int as_step_counters_host(as_env_t* env, int32_t* out_host, void* stream) {
  if (!env || !out_host) return fail(AS_ERR_INVALID, "as_step_counters_host: null argument");
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  HIP_TRY(hipMemcpyAsync(out_host, env->counters_dev + as::kCntBank * env->last_bank, 4 * sizeof(int32_t),
                         hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return AS_OK;
}

int as_get_curriculum_host(as_env_t* env, int32_t* level_host) {
  if (!env || !level_host) return fail(AS_ERR_INVALID, "as_get_curriculum_host: null argument");
  HIP_TRY(hipMemcpy(level_host, env->st.curriculum, sizeof(int32_t), hipMemcpyDeviceToHost));
  return AS_OK;
}

}  // extern "C"
