// TEST INFRASTRUCTURE: the one translation unit that holds the emulator's scheduler.
#define EEG_SIMT_EMU_IMPL
#include "simt_emu.h"

// the product's event-based kernel timer (csrc/prof.cpp) has nothing to time here; the emulator's recorder keeps what the tests read
// from it: which launch role went out how often, as which kernel (the symbol of the host function EEG_LAUNCH_P was handed, spelled
// as the product's report spells it).  Times are reported as zero.
#include <cxxabi.h>
#include <dlfcn.h>

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "prof.h"
namespace eeg {
namespace {
struct EmuRec { std::string name; const void* kern; int count; };
bool g_on = false;
std::string g_prefix;
std::vector<EmuRec> g_recs;
std::string kernel_symbol(const void* kern) {
    Dl_info info;
    if (kern == nullptr || dladdr(kern, &info) == 0 || info.dli_sname == nullptr) return "?";
    int st = 0;
    char* dem = abi::__cxa_demangle(info.dli_sname, nullptr, nullptr, &st);
    std::string sym = (st == 0 && dem != nullptr) ? dem : info.dli_sname;
    free(dem);
    if (sym.rfind("void ", 0) == 0) sym = sym.substr(5);
    int depth = 0;
    for (size_t i = 0; i < sym.size(); ++i) {
        depth += sym[i] == '<';
        depth -= sym[i] == '>';
        if (sym[i] == '(' && depth == 0) { sym = sym.substr(0, i); break; }
    }
    if (sym.rfind("eeg::", 0) == 0) sym = sym.substr(5);
    return sym;
}
}  // namespace
void prof_begin(const char* name, hipStream_t, const void* kern) {
    if (!g_on) return;
    const std::string full = g_prefix + name;
    for (auto& r : g_recs)
        if (r.name == full && r.kern == kern) { ++r.count; return; }
    g_recs.push_back({full, kern, 1});
}
bool prof_is_on() { return g_on; }
void prof_end(hipStream_t) {}
void prof_set_prefix(const char* prefix) { g_prefix = prefix != nullptr ? prefix : ""; }
void prof_enable(bool on) { g_on = on; }
size_t prof_report(char* buf, size_t cap) {
    std::string out;
    for (auto& r : g_recs) out += r.name + " " + std::to_string(r.count) + " 0.000000 " + kernel_symbol(r.kern) + "\n";
    g_recs.clear();
    if (out.size() + 1 > cap) return out.size() + 1;
    memcpy(buf, out.c_str(), out.size() + 1);
    return 0;
}
}  // namespace eeg
