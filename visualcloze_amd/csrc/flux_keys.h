// The state_dict() keys a VcFluxConfig implies (FluxLoraWrapper, models/model.py:154-175: Flux with a LoRA pair on every Linear),
// their shapes, and what vc_flux_load_* needs to know about each.  Host code only, nothing from HIP: flux_weights.hip uses it for
// vc_flux_load_key / vc_flux_load_tensor / vc_flux_load_bytes / vc_flux_load_finish, tests/c_abi/flux_keys_check.cpp runs it alone.
#pragma once
#include <stdint.h>
#include <string>
#include <unordered_map>
#include <vector>
#include "../../include/vcloze_hip.h"

namespace vckeys {

constexpr int MAX_RANK = 512;       // vc_lora_merge's limit

enum Kind { WEIGHT, BIAS, LORA_A, LORA_B, LORA_B_BIAS, SCALE };

// an nn.Linear by reference module path; mod_off >= 0: its first row in the stacked modulation matrix
struct Linear {
  std::string name;
  int out = 0, in = 0;
  bool qkv = false;         // rows [0, 3 * hidden) are stored head-permuted (every *_attn.qkv, every linear1)
  int64_t mod_off = -1;
  int key0 = 0;             // its keys are key0 + WEIGHT .. key0 + LORA_B_BIAS of Table::keys
};
// a key of the state_dict: shape[d] == -1 is the LoRA rank (free, 0 .. MAX_RANK)
struct Key {
  std::string name;
  Kind kind = WEIGHT;
  int owner = 0;            // index into Table::linears, or into Table::scales for a SCALE
  int64_t shape[2] = {0, 0};
  int ndim = 1;
};
struct Table {
  std::vector<Linear> linears;          // in state_dict order
  std::vector<std::string> scales;      // the QK-norm scale keys, in state_dict order
  std::vector<Key> keys;                // every key, in state_dict order
  std::unordered_map<std::string, int> index;
  int64_t n_mod = 0;
};

Table build(const VcFluxConfig& cfg);
// the index of `key` in t.keys, or -1
int find(const Table& t, const char* key);
// key `index` -> name (truncated to namelen - 1 characters and terminated), shape, ndim; VC_ERR_ARG past the end or on null / empty buffers
int describe(const Table& t, int index, char* name, int namelen, int64_t* shape, int32_t* ndim, char* err, int errlen);
// VC_OK when `shape` is the key's (a rank dimension: 0 .. MAX_RANK); else VC_ERR_ARG naming the key, what was expected and what came
int check_shape(const Key& k, const int64_t* shape, int ndim, char* err, int errlen);
// bytes of the prepared set (the formula of include/vcloze_hip.h, vc_flux_load_bytes)
int64_t arena_bytes(const Table& t, int hidden);

}  // namespace vckeys
