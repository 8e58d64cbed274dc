// Internal helpers shared by the translation units of libjsg.so (not part of the C-ABI).
#pragma once
#include <hip/hip_runtime_api.h>

#include <string>
#include <vector>

#include "../../include/jsg.h"

namespace jsg {

// last error text of the calling thread (jsg_last_error(NULL)); engines keep their own copy too
std::string& tls_error();
int jsg_fail(int code, const char* what);
int jsg_fail_hip(hipError_t err, const char* where);

// jsg_kernels.hip: compute units of a device (read once per device), the device a plan was created on
int cu_count_of_device(int dev);
int plan_device(const jsg_plan* plan);

}  // namespace jsg

// jsg_kernels.hip: the plan_select that pins every launch of a strided call (n_batches >= 1) to the plan of the whole call;
// jsg_filterbank.hip pins its STFT chunks with it (defined inside the C-ABI block of jsg_kernels.hip; hidden like every internal symbol)
extern "C" int strided_plan_select(const jsg_plan* plan, const jsg_stft_args* g, int n_batches, int n_cu);

// A filterbank on the device (jsg_filterbank_host.cpp creates it, jsg_filterbank.hip applies it): the CSR of jsg_filterbank_build,
// band descriptors as three int arrays of n_bands entries (first bin, bin count, weight offset) followed by the weights, one allocation
struct jsg_filterbank {
    int n = 0;
    int n_bands = 0;
    int device = -1;
    long long nnz = 0;
    int* d_desc = nullptr;      // first_bin[n_bands], n_bins[n_bands], offset[n_bands], then nnz floats of weights
    const float* d_w = nullptr;
    std::vector<int> first, count, offset;   // host copy (jsg_filterbank_weights)
    std::vector<float> w;
};
