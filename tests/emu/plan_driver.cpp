// TEST INFRASTRUCTURE ONLY -- runs conv_plan.hpp's pure launch planner on the host for tests/test_conv_plan.py.  One query per input line:
//   P ks stride pad reflect cin cout npad kpad form N H W csplit transform nprod fin_counter cus  -> plan_conv with the default request
//   R <the P fields> kernel rows width alt sched chunk xcd_gn [x2_nmod]                           -> plan_conv with that request (x2_nmod: images of the second tensor, default 1)
//   T kernel tile                                                                                 -> decode_tile_code
//   V variant                                                                                     -> decode_bench_variant
//   C code                                                                                        -> decode_head_code
//   H B tiles_x hh cus                                                                            -> head_rows
// One output line per query: space-separated integers, or "ERR <message>".
#include <iostream>
#include <sstream>
#include <string>

#include "../../wacv23_tsnet_amd/csrc/conv_plan.hpp"

using namespace tsnet;

static void put_request(std::ostream& o, const ConvRequest& r) {
    o << (int)r.kernel << ' ' << r.rows << ' ' << r.width << ' ' << (int)r.alt << ' ' << (int)r.sched << ' ' << r.chunk << ' ' << r.chunk_cap << ' '
      << r.abl << ' ' << r.opt << ' ' << r.xcd_gn;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::ostringstream o;
        char q = 0;
        in >> q;
        try {
            if (q == 'P' || q == 'R') {
                ConvShape s;
                ConvRequest r;
                int transform = 0, fin = 0, cus = 0, kernel = 0, alt = 0, sched = 0;
                in >> s.ks >> s.stride >> s.pad >> s.reflect >> s.cin >> s.cout >> s.npad >> s.kpad >> s.form >> s.N >> s.H >> s.W >> s.csplit >> transform
                   >> s.nprod >> fin >> cus;
                s.transform = transform != 0; s.fin_counter = fin != 0;
                if (q == 'R') {
                    in >> kernel >> r.rows >> r.width >> alt >> sched >> r.chunk >> r.xcd_gn;
                    if (!in || kernel < 0 || kernel > 2 || sched < 0 || sched > 2) throw std::invalid_argument("R: seven request fields, kernel and sched 0 to 2");
                    r.kernel = static_cast<ConvKernel>(kernel); r.alt = alt != 0; r.sched = static_cast<ConvSched>(sched);
                    int nmod = 0;
                    if (in >> nmod) s.x2_nmod = nmod;
                }
                const ConvPlan p = plan_conv(s, r, cus);
                o << (int)p.family << ' ' << p.rows << ' ' << p.width << ' ' << (int)p.side_by_side << ' ' << (int)p.sched << ' ' << p.w1_chunk << ' '
                  << p.w1_tab2 << ' ' << p.xcd_gn << ' ' << p.tpi << ' ' << p.tiles_m << ' ' << p.tiles_n << ' ' << (int)p.fin;
            } else if (q == 'T') {
                int kernel = 0, tile = 0;
                in >> kernel >> tile;
                put_request(o, decode_tile_code(kernel, tile));
            } else if (q == 'V') {
                int v = 0;
                in >> v;
                const BenchVariant b = decode_bench_variant(v);
                put_request(o, b.req);
                o << ' ' << b.nprod << ' ' << b.form << ' ' << (int)b.cold;
            } else if (q == 'C') {
                int code = 0;
                in >> code;
                const HeadRequest h = decode_head_code(code);
                o << (int)h.composite << ' ' << h.rows;
            } else if (q == 'H') {
                int B = 0, tiles_x = 0, hh = 0, cus = 0;
                in >> B >> tiles_x >> hh >> cus;
                o << head_rows(B, tiles_x, hh, cus);
            } else {
                o << "ERR unknown query";
            }
        } catch (const std::invalid_argument& e) {
            o.str("");
            o << "ERR " << e.what();
        }
        std::cout << o.str() << '\n';
    }
    return 0;
}
