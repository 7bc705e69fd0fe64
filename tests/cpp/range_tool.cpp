// Test driver of IndexIVF_HNSW::range_search through the class surface (tests/test_gpu_range_class.py builds it with
// g++).  KIND is ivf (IndexIVF_HNSW) or grouping (IndexIVF_HNSW_Grouping).
//   range_tool KIND d nc code_size nsubc centroids info edges pq norm_pq opq|- in.index queries.fvecs nq nprobe
//              max_codes ef pruning radius_bits labels.u32|- deny out.bin
//       range_search; with labels: set_id_filter(labels, deny), range_search; clear_id_filter(), range_search.
//       out.bin, per round: lims [nq + 1] (uint64), distances [total] (float), labels [total] (int64).
// radius_bits is the radius as the decimal value of its 32 float bits; labels.u32 is a raw uint32 array.
#include <ivf-hnsw/IndexIVF_HNSW_Grouping.h>

#include <cstdio>
#include <cstring>
#include <fstream>
#include <stdexcept>
#include <string>
#include <vector>

using namespace ivfhnsw;

static std::vector<IndexIVF_HNSW::idx_t> read_u32(const char *path)
{
    std::ifstream in(path, std::ios::binary);
    if (!in)
        throw std::runtime_error(std::string("cannot open ") + path);
    in.seekg(0, std::ios::end);
    const size_t n = (size_t)in.tellg() / sizeof(uint32_t);
    in.seekg(0);
    std::vector<IndexIVF_HNSW::idx_t> v(n);
    in.read(reinterpret_cast<char *>(v.data()), n * sizeof(uint32_t));
    return v;
}

int main(int argc, char **argv)
try {
    if (argc != 23)
        throw std::runtime_error("usage: see the head of range_tool.cpp");
    const std::string kind = argv[1];
    const size_t d = atol(argv[2]), nc = atol(argv[3]), cs = atol(argv[4]), nsubc = atol(argv[5]);
    const char *centroids = argv[6], *info = argv[7], *edges = argv[8], *ppq = argv[9], *pnorm = argv[10], *popq = argv[11],
               *pindex = argv[12], *pqueries = argv[13];
    const size_t nq = atol(argv[14]), nprobe = atol(argv[15]), max_codes = atol(argv[16]), ef = atol(argv[17]);
    const bool pruning = atoi(argv[18]) != 0;
    const uint32_t rbits = (uint32_t)strtoul(argv[19], nullptr, 10);
    float radius;
    memcpy(&radius, &rbits, sizeof(radius));
    const char *plab = argv[20];
    const bool deny = atoi(argv[21]) != 0;
    IndexIVF_HNSW *index;
    if (kind == "grouping")
        index = new IndexIVF_HNSW_Grouping(d, nc, cs, 8, nsubc);
    else if (kind == "ivf")
        index = new IndexIVF_HNSW(d, nc, cs, 8);
    else
        throw std::runtime_error("KIND must be ivf or grouping");
    index->build_quantizer(centroids, info, edges, 16, 500);
    index->do_opq = strcmp(popq, "-") != 0;
    delete index->pq;
    index->pq = faiss::read_ProductQuantizer(ppq);
    if (index->do_opq)
        index->opq_matrix = dynamic_cast<faiss::LinearTransform *>(faiss::read_VectorTransform(popq));
    delete index->norm_pq;
    index->norm_pq = faiss::read_ProductQuantizer(pnorm);
    index->read(pindex);
    if (index->do_opq)
        index->rotate_quantizer();
    index->nprobe = nprobe;
    index->max_codes = max_codes;
    index->quantizer->efSearch = ef;
    if (auto *g = dynamic_cast<IndexIVF_HNSW_Grouping *>(index))
        g->do_pruning = pruning;
    std::vector<float> q(nq * d);
    {
        std::ifstream in(pqueries, std::ios::binary);
        readXvec<float>(in, q.data(), d, nq);
    }
    FILE *f = fopen(argv[22], "wb");
    if (!f)
        throw std::runtime_error("cannot write the result file");
    auto round = [&]() {
        std::vector<size_t> lims;
        std::vector<float> dist;
        std::vector<long> lab;
        index->range_search(nq, q.data(), radius, lims, dist, lab);
        if (lims.size() != nq + 1 || dist.size() != lims[nq] || lab.size() != lims[nq])
            throw std::runtime_error("range_search: sizes of the three arrays do not agree");
        fwrite(lims.data(), sizeof(size_t), lims.size(), f);
        fwrite(dist.data(), sizeof(float), dist.size(), f);
        fwrite(lab.data(), sizeof(long), lab.size(), f);
    };
    round();
    if (strcmp(plab, "-") != 0) {
        const std::vector<IndexIVF_HNSW::idx_t> lab = read_u32(plab);
        index->set_id_filter(lab.size(), lab.data(), deny);
        round();
        index->clear_id_filter();
        round();
    }
    fclose(f);
    delete index;
    return 0;
} catch (const std::exception &e) {
    fprintf(stderr, "range_tool: %s\n", e.what());
    return 1;
}
