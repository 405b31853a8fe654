// The named-tensor table of a network handle (Vocoder, HifiGan, DVector, MosNet): one zero-filled device block of float32, every tensor at
// an offset rounded to 4 floats (16-byte rows for float4 loads), found by name.  The table is built once at init and filled by the C
// `*_load` entries; what a handle does after a tensor arrived (re-pack an image, mark derived weights stale) is the handle's own business,
// so load() hands back the tensor it hit.  Host-side bookkeeping only.
#pragma once
#include <string>
#include <vector>

#include "devres.h"

namespace mtts {

class ParamTable {
public:
    struct Tensor { std::string name; long long off, numel; bool loaded; };
    std::vector<Tensor> tensors;
    float* data = nullptr;
    long long n_params = 0;   // floats of the block, the rounding included

    void add(const std::string& name, long long numel) { tensors.push_back(Tensor{name, n_params, numel, false}); n_params += (numel + 3) & ~3LL; }
    long long find(const std::string& name) const { for (auto& t : tensors) if (t.name == name) return t.off; return -1; }
    float* ptr(const std::string& name) const { const long long o = find(name); return o < 0 ? nullptr : data + o; }
    hipError_t alloc(DevHeap& mem) { return mem.alloc_zeroed(data, (size_t)n_params * sizeof(float)); }

    // The tensor `name` if it has `numel` floats, else nullptr with the refusal in `error`; `kind` names the network in the message.
    Tensor* check(const char* name, long long numel, const char* kind, std::string& error) {
        for (auto& t : tensors)
            if (t.name == name) {
                if (t.numel == numel) return &t;
                error = std::string("size mismatch for ") + name + ": " + std::to_string(numel) + " floats given, " + std::to_string(t.numel) + " expected";
                return nullptr;
            }
        error = std::string("unknown ") + kind + " tensor " + name;
        return nullptr;
    }
    // host -> device; nullptr (message in `error`) when the arguments, the name, the size or the copy are refused: nothing has changed then
    Tensor* load(const char* name, const float* host, long long numel, const char* kind, std::string& error) {
        if (!name || !host) { error = std::string(kind) + " load: NULL argument"; return nullptr; }
        Tensor* t = check(name, numel, kind, error);
        if (!t) return nullptr;
        const hipError_t e = hipMemcpy(data + t->off, host, (size_t)numel * sizeof(float), hipMemcpyHostToDevice);
        if (e != hipSuccess) { error = std::string("upload of ") + name + ": " + hipGetErrorString(e); return nullptr; }
        t->loaded = true;
        return t;
    }
};

}  // namespace mtts
