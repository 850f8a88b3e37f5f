// map_slices.cpp -- the slices sfa_plan.hpp cuts a batch of event-map rows into (tests/test_event_maps_cpu.py).
// stdin: one case per line, "name budget qlen:m qlen:m ..."; stdout per case: "name slices=a,b|c,d|... host=e,f bytes=x|y|... off=..."
// (row numbers per slice, rows left to the host, bytes of scratch every slice takes, byte offset of every device row).
#include <cstdint>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "sfa_plan.hpp"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string name, kv;
        int64_t budget = 0;
        in >> name >> budget;
        std::vector<int32_t> qlen, m;
        while (in >> kv) {
            qlen.push_back(std::stoi(kv.substr(0, kv.find(':'))));
            m.push_back(std::stoi(kv.substr(kv.find(':') + 1)));
        }
        const sfa::MapSlices s = sfa::plan_map_slices(qlen.data(), m.data(), static_cast<int32_t>(qlen.size()), budget);
        std::cout << name << " slices=";
        for (size_t i = 0; i + 1 < s.slice_begin.size(); ++i) {
            if (i) std::cout << "|";
            for (int32_t o = s.slice_begin[i]; o < s.slice_begin[i + 1]; ++o) std::cout << (o > s.slice_begin[i] ? "," : "") << s.order[o];
        }
        std::cout << " host=";
        for (size_t i = 0; i < s.host_rows.size(); ++i) std::cout << (i ? "," : "") << s.host_rows[i];
        std::cout << " bytes=";
        for (size_t i = 0; i + 1 < s.slice_begin.size(); ++i) {
            int64_t end = 0;
            for (int32_t o = s.slice_begin[i]; o < s.slice_begin[i + 1]; ++o)
                end = std::max(end, s.mv_off[o] + sfa::map_row_bytes(qlen[s.order[o]], m[s.order[o]]));
            std::cout << (i ? "|" : "") << end;
        }
        std::cout << " off=";
        for (size_t o = 0; o < s.order.size(); ++o) std::cout << (o ? "," : "") << s.mv_off[o];
        std::cout << "\n";
    }
    return 0;
}
