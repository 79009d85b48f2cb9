// nrs_optimizer.h -- what nrs_api_optimizer.cpp, nrs_optimizer.hip and nrs_api_model.cpp share: the argument block and launchers of the optimiser step
// (include/nrs.h, "optimiser"), and the two doors through which an optimiser bound to a model hands it new parameters.  Not part of the public ABI.
#pragma once
#include "../../include/nrs.h"

struct nrs_model;

namespace nrs {

constexpr uint32_t kAdamTableMax = 65536;   // entries of the bias table at most (nrs_adam_bias_table refuses betas that need more)
constexpr uint32_t kAdamTableLds = 4096;    // entries at most for the step to stage the table in LDS (16 KB); a longer one is read through L2
constexpr size_t kAdamMaxParams = 1ull << 31; // element indices are 32 bits wide in the kernels

// Where the fp16 copy of element i lives: h_lo[i] for i < split, h_hi[i - split] otherwise.  An unbound optimiser has split == n (one array); one bound to a
// model has split == the number of MLP weights, h_lo its own small buffer and h_hi the model's resident hash table.
struct Fp16Dest {
	uint16_t* h_lo;
	uint16_t* h_hi;
	uint32_t split;
};

struct AdamStepArgs {
	uint32_t n, n_matrix;
	float* grad;             // [n], any 4-byte alignment; written only with zero_grad
	float *master, *m, *v;   // [n] each, 16-byte aligned (the optimiser's own allocations)
	uint32_t* steps;         // [n]
	float* ema;              // [n]; touched only when ema_on
	Fp16Dest h;
	const float* table;      // [t_sat + 1]: table[t] = bias(t) for t in 1..t_sat, table[0] unused
	uint32_t t_sat;
	float loss_scale, beta1, beta2, one_minus_beta1, one_minus_beta2, epsilon, l2_reg;
	float lr_matrix, lr_other; // learning_rate * 1, learning_rate * non_matrix_lr_factor (fp32 products)
	float ema_a, ema_b;
	uint32_t zero_grad, ema_on;
	uint32_t variant;        // measurement knobs (NRS_OPTIMIZER_VARIANT): 1 = the EMA in a launch of its own, 2 = the bias table read through L2 instead of staged in LDS
};

int launch_adam_step(const AdamStepArgs& a, void* stream);
// ema[i] = master[i] and fp16(i) = round-to-nearest-even(master[i]) for every i (nrs_optimizer_set_weights)
int launch_adam_init(uint32_t n, const float* master, float* ema, const Fp16Dest& h, void* stream);
int launch_round_fp16(uint32_t n, const float* in, uint16_t* out, void* stream);

// nrs_api_model.cpp: the halves of nrs_model_set_params_device an optimiser needs when the hash table has been written in place.
void model_param_counts(const nrs_model* m, uint32_t* n_mlp, size_t* n_params);
int model_mlp_from_device(nrs_model* m, const uint16_t* d_mlp_fp16, void* stream); // MFMA fragments from the blob's leading MLP weights (builds the permutation on first use)
int model_grid_written(nrs_model* m, void* stream);                                // have_params, then the cell records if the model keeps any; never waits
uint16_t* model_grid_fp16(nrs_model* m);                                           // the resident table as fp16 pairs, in the blob's order

} // namespace nrs
