// Test driver of IndexIVF_HNSW::set_id_filter / clear_id_filter through the class surface (tests/test_gpu_filter_class.py
// builds it with g++).  KIND is ivf (IndexIVF_HNSW) or grouping (IndexIVF_HNSW_Grouping).
//   filter_tool KIND d nc code_size nsubc centroids info edges pq norm_pq opq|- in.index queries.fvecs nq k nprobe
//               max_codes ef pruning labels.u32 deny add.fvecs|- add_first_id out.bin out.index
//       search, set_id_filter(labels, deny), search, add_batch(add rows, ids add_first_id ..) when given, search,
//       invalidate_device(), search, clear_id_filter(), search, write.
//       out.bin: labels [5][nq][k] (int64), distances [5][nq][k] (float).
// labels.u32 is a raw uint32 array.
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
    if (argc != 26)
        throw std::runtime_error("usage: see the head of filter_tool.cpp");
    const std::string kind = argv[1];
    const size_t d = atol(argv[2]), nc = atol(argv[3]), cs = atol(argv[4]), nsubc = atol(argv[5]);
    const char *centroids = argv[6], *info = argv[7], *edges = argv[8], *ppq = argv[9], *pnorm = argv[10], *popq = argv[11],
               *pindex = argv[12], *pqueries = argv[13];
    const size_t nq = atol(argv[14]), k = atol(argv[15]), nprobe = atol(argv[16]), max_codes = atol(argv[17]),
                 ef = atol(argv[18]);
    const bool pruning = atoi(argv[19]) != 0;
    const std::vector<IndexIVF_HNSW::idx_t> lab = read_u32(argv[20]);
    const bool deny = atoi(argv[21]) != 0;
    const char *padd = argv[22];
    const IndexIVF_HNSW::idx_t add_first = (IndexIVF_HNSW::idx_t)atol(argv[23]);
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
    const size_t per = nq * k;
    std::vector<long> out_l(5 * per);
    std::vector<float> out_d(5 * per);
    size_t round = 0;
    auto search = [&]() {
        index->search_batch(nq, k, q.data(), out_d.data() + round * per, out_l.data() + round * per);
        round++;
    };
    search();
    index->set_id_filter(lab.size(), lab.data(), deny); // the device copy is current: installed at once
    search();
    if (strcmp(padd, "-") != 0) {
        std::ifstream bin(padd, std::ios::binary);
        bin.seekg(0, std::ios::end);
        const size_t nb = (size_t)bin.tellg() / (sizeof(int) + d * sizeof(float));
        bin.seekg(0);
        std::vector<float> base(nb * d);
        readXvec<float>(bin, base.data(), d, nb);
        std::vector<IndexIVF_HNSW::idx_t> ids(nb);
        for (size_t i = 0; i < nb; i++)
            ids[i] = add_first + (IndexIVF_HNSW::idx_t)i;
        index->add_batch(nb, base.data(), ids.data());
    }
    search();
    index->invalidate_device(); // the next search uploads everything again, the filter with it
    search();
    index->clear_id_filter();
    search();
    FILE *f = fopen(argv[24], "wb");
    if (!f)
        throw std::runtime_error("cannot write the result file");
    fwrite(out_l.data(), sizeof(long), out_l.size(), f);
    fwrite(out_d.data(), sizeof(float), out_d.size(), f);
    fclose(f);
    index->write(argv[25]);
    delete index;
    return 0;
} catch (const std::exception &e) {
    fprintf(stderr, "filter_tool: %s\n", e.what());
    return 1;
}
